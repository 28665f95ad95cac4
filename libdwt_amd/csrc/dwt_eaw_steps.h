// dwt_eaw_steps.h -- what the edge-avoiding 5/3 (dwt_eaw.hip) and 9/7 (dwt_eaw97.hip) kernels share: the weight of a
// sample pair, the place of a sample in a line, the alpha mode and the grid of the line kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

namespace dwt {

// dwt_eaw_w (src/libdwt.c:11070, src/eaw-experimental.c:56).  mode 0: alpha == 0 (powf(x, 0) == 1 for every x); mode 1:
// alpha == 1 (powf(x, 1) == x for every float); mode 2: any other alpha, pow in double rounded once to float (within
// 1 ulp of glibc's powf).
static __device__ __forceinline__ float eaw_weight(float n, float m, float alpha, int mode)
{
	const float eps = 1.0e-5f;
	const float d = fabsf(n - m);
	float p;
	if (mode == 0)
		p = 1.f;
	else if (mode == 1)
		p = d;
	else
		p = (float)pow((double)d, (double)alpha);
	return 1.f / (p + eps);
}

// Where sample i of a line sits: Mallat (L at i/2, H at hoff + i/2) or interleaved (at i).
static __device__ __forceinline__ long eaw_pos(int i, int hoff) { return hoff < 0 ? i : (i & 1) ? hoff + (i >> 1) : (i >> 1); }

static inline int eaw_mode(float alpha) { return alpha == 0.f ? 0 : alpha == 1.f ? 1 : 2; }

static inline dim3 eaw_grid(long threads)
{
	long b = (threads + 255) / 256;
	return dim3((unsigned)(b < 65536 ? (b > 0 ? b : 1) : 65536));
}

} // namespace dwt
