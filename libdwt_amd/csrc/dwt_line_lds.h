// dwt_line_lds.h -- the load that opens the kernels which keep a whole line in LDS (k_line_levels, dwt_line1d.hip;
// k_swt_lines, dwt_swt1d.hip).
#pragma once

namespace dwt {

// The line of N floats at `s`, elements `es` bytes apart, into LDS by the `nt` threads that work on it (this one is t):
// 16 B per lane where the launcher found the line dense and 16-byte aligned (vec), one element per lane otherwise.
static __device__ __forceinline__ void line_to_lds(float *lds, const char *s, int N, long es, int t, int nt, bool vec)
{
	if (vec) {
		const int n4 = N >> 2;
		for (int i = t; i < n4; i += nt)
			*(float4 *)(lds + 4 * i) = *(const float4 *)(s + 16l * i);
		for (int i = 4 * n4 + t; i < N; i += nt)
			lds[i] = *(const float *)(s + 4l * i);
	} else {
		for (int i = t; i < N; i += nt)
			lds[i] = *(const float *)(s + (long)i * es);
	}
}

} // namespace dwt
