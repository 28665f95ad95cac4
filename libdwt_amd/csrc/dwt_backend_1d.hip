// dwt_backend_1d.hip -- the 1-D drivers: dwt_cdf97_1f_s / _1i_s, dwt_cdf53_1f_s / _1i_s and the row-wise
// dwt_cdf{97,53}_2f1_s (src/libdwt.c:16025, :15766, :16097, :15835, :15965, :15995) on the device.
//
// Dense lines of up to N1D_MAX samples run every level in ONE launch of k_line_levels (dwt_line1d.hip), whatever the
// depth.  Longer lines run the levels whose input exceeds the cap as exact per-level passes (generic_pass), the rest in
// one k_line_levels launch over the L prefix; the inverse is the mirror.  Sparse frames (size_o != size_i), and every
// call under option "generic" / accel 1, run the reference's loop level by level: one exact line pass plus its zero fills.
#include "dwt_backend.h"

namespace dwtb {

// levels whose input (forward) / output (inverse) line is longer than the fused kernel takes: they run as line passes
static int long_levels(int so, int J)
{
	int j = 0;
	while (j < J && ceil_div_pow2(so, j) > N1D_MAX)
		j++;
	return j;
}

static int fused_launch(Wavelet w, bool inverse, const char *s, char *d, long ls, long es, int n_lines, int N, int levels)
{
	return launched(launch_line_levels(w, inverse, s, d, ls, es, n_lines, N, levels, g.stream), "1-D", "level");
}

// Forward, in place on `d` (lines of dense 4-byte elements, row pitch d.sx), J levels already clamped.
static int forward_levels(Wavelet w, Img d, int n_lines, int so, int si, int J, int zero_padding)
{
	const bool fused = so == si && !g.force_generic;
	const int jg = fused ? long_levels(so, J) : J; // levels 0 .. jg-1 as line passes
	for (int j = 0; j < jg; j++) {
		const int so_src = ceil_div_pow2(so, j), so_dst = ceil_div_pow2(so, j + 1), si_src = ceil_div_pow2(si, j);
		// (size_o_src > 1 holds at every level below the clamped depth: src/libdwt.c:16060)
		if (generic_pass(w, false, true, d, d, so_src, n_lines, n_lines, si_src, so_dst))
			return 1;
		if (zero_padding) {
			// dwt_zero_padding_f_stride_s (src/libdwt.c:12118): L beyond ceil(N/2), H beyond floor(N/2)
			const int nl = (si_src + 1) >> 1, nh = si_src >> 1;
			if (zero_rect(d, nl, 0, so_dst - nl, n_lines) || zero_rect(d, so_dst + nh, 0, (so_src - so_dst) - nh, n_lines))
				return 1;
		}
	}
	if (jg < J)
		return fused_launch(w, false, d.p, d.p, d.sx, d.es, n_lines, ceil_div_pow2(so, jg), J - jg);
	return 0;
}

// Inverse, in place on `d`: the reference's levels J .. 1 (level j rebuilds ceil(so / 2^(j-1)) samples).
static int inverse_levels(Wavelet w, Img d, int n_lines, int so, int si, int J, int zero_padding)
{
	const bool fused = so == si && !g.force_generic;
	const int jg = fused ? long_levels(so, J) : J; // the finest jg levels as line passes
	if (jg < J && fused_launch(w, true, d.p, d.p, d.sx, d.es, n_lines, ceil_div_pow2(so, jg), J - jg))
		return 1;
	for (int j = jg; j >= 1; j--) {
		const int so_src = ceil_div_pow2(so, j), so_dst = ceil_div_pow2(so, j - 1), si_dst = ceil_div_pow2(si, j - 1);
		if (generic_pass(w, true, true, d, d, so_dst, n_lines, n_lines, si_dst, so_src))
			return 1;
		// dwt_zero_padding_i_stride_s (src/libdwt.c:12199)
		if (zero_padding && zero_rect(d, si_dst, 0, so_dst - si_dst, n_lines))
			return 1;
	}
	return 0;
}

int transform1d(Wavelet w, bool inverse, const void *src, void *dst, long line_stride, long elem_stride, int n_lines,
	int so, int si, int *jp, int zero_padding)
{
	// the level count, clamped as the reference clamps it
	const int j_limit = ceil_log2(so);
	int J;
	if (!inverse) {
		if (*jp < 0 || *jp > j_limit)
			*jp = j_limit; // src/libdwt.c:16050-16053
		J = *jp;
	} else {
		J = j_limit; // src/libdwt.c:15795-15798
		if (*jp >= 0 && *jp < J)
			J = *jp;
	}
	if (n_lines == 0 || so == 0)
		return 0;
	if (n_lines == 1)
		line_stride = (long)so * elem_stride; // (not used: one line)
	const bool dev = dwt_hip_is_device_pointer(dst);
	if (dev != (bool)dwt_hip_is_device_pointer(src))
		return fail("src and dst must both be host or both be device pointers");
	if (J == 0 && src == dst)
		return 0;

	// device lines, dense frame, one launch for all levels: straight from src to dst, any element stride (the frame's
	// every element is written)
	if (dev && J >= 1 && so == si && so <= N1D_MAX && !g.force_generic && elem_stride % 4 == 0 && line_stride % 4 == 0 &&
		(uintptr_t)src % 4 == 0 && (uintptr_t)dst % 4 == 0)
		return fused_launch(w, inverse, (const char *)src, (char *)dst, line_stride, elem_stride, n_lines, so, J);

	// device lines of dense, aligned elements that do not overlap: in place on dst, after a copy when out of place
	if (dev && elem_stride == 4 && line_stride % 4 == 0 && (n_lines == 1 || line_stride >= 4l * so) &&
		(uintptr_t)src % 4 == 0 && (uintptr_t)dst % 4 == 0) {
		const Img d{(char *)dst, n_lines == 1 ? align_up(4l * so, 4) : line_stride, 4};
		if (src != dst && copy_rect(d, 0, 0, Img{(char *)src, d.sx, 4}, 0, 0, so, n_lines))
			return 1;
		return inverse ? inverse_levels(w, d, n_lines, so, si, J, zero_padding) : forward_levels(w, d, n_lines, so, si, J, zero_padding);
	}

	// anything else -- host memory, strided elements -- takes the staging detour (dwt_backend.h) and is transformed in
	// place in the dense device frame
	const Frame fs{(void *)src, line_stride, elem_stride, 4, so, n_lines, dev};
	if (frame_check(fs))
		return 1;
	Img A;
	if (frame_stage(fs, g.frame_a, &A))
		return 1;
	const long pitch = A.sx;
	int rc = 0;
	if (J >= 1 && so == si && so <= N1D_MAX && !g.force_generic)
		rc = fused_launch(w, inverse, A.p, A.p, pitch, 4, n_lines, so, J);
	else if (J >= 1)
		rc = inverse ? inverse_levels(w, A, n_lines, so, si, J, zero_padding) : forward_levels(w, A, n_lines, so, si, J, zero_padding);
	if (rc)
		return rc;
	return frame_unpack(Frame{dst, line_stride, elem_stride, 4, so, n_lines, dev}, A.p, pitch);
}

} // namespace dwtb
