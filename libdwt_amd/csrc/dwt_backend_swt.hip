// dwt_backend_swt.hip -- the stationary wavelet transform of row batches (swt_cdf97_f_ex_stride_s /
// swt_cdf53_f_ex_stride_s, src/swt.c) on the device, and its C-ABI (include/libdwt_hip.h).
//
// Device lines of dense elements and up to N1D_MAX samples run every level in ONE launch of k_swt_lines (dwt_swt1d.hip).
// Longer lines, strided elements, and every call under option "swt_fused" = 0 run one exact k_swt_level launch per level,
// the L chain ping-ponged through library scratch.  Host memory takes the staging detour (dwt_backend.h): the lines
// into a dense device image, transformed there into dense device planes, each plane spread back.
#include "dwt_backend.h"

#include <climits>

namespace dwtb {

bool swt_fused_ok(const void *src, long ls, long es, int N)
{
	return g.swt_fused && N <= N1D_MAX && es == 4 && ls % 4 == 0 && (uintptr_t)src % 4 == 0;
}

// Device memory on every side.  H of level l of line y at dst_h + l*plane_stride + y*dls, elements h_es bytes apart; L
// likewise by l_mode.  Level l has dilation 1 << (level0 + l).  dst_h may be null where the level passes run (no H stored).
int swt_device(Wavelet w, const char *src, long ls, long es, int n_lines, int N, int level0, int levels, char *dst_h, long h_es,
	char *dst_l, long l_es, int l_mode, long plane_stride, long dls, int border)
{
	if (n_lines <= 0 || levels <= 0 || N <= 0)
		return 0;
	if (check_dev_align({src, dst_h, l_mode ? dst_l : nullptr}, {es, ls, h_es, plane_stride, dls, l_mode ? l_es : 0}))
		return 1;
	if (dst_h && swt_fused_ok(src, ls, es, N) && h_es == 4 && (!l_mode || l_es == 4)) {
		SwtLineArgs a{};
		a.src = src;
		a.line_stride = ls;
		a.n_lines = n_lines;
		a.N = N;
		a.level0 = level0;
		a.levels = levels;
		a.vec = ls % 16 == 0 && (uintptr_t)src % 16 == 0;
		a.dst_h = dst_h;
		a.dst_l = dst_l;
		a.plane_stride = plane_stride;
		a.dst_line_stride = dls;
		a.l_mode = l_mode;
		a.border = border;
		return launched(launch_swt_lines(w, false, a, g.stream), "SWT", "line");
	}
	// level by level: the L chain through two dense scratch images
	const long pitch = 4l * N;
	char *pp[2] = {nullptr, nullptr};
	if (levels > 1) {
		if (grow(g.swt_ws, (size_t)2 * pitch * n_lines))
			return 1;
		pp[0] = (char *)g.swt_ws.p;
		pp[1] = pp[0] + (size_t)pitch * n_lines;
	}
	for (int l = 0; l < levels; l++) {
		const bool last = l == levels - 1;
		SwtLevelArgs a{};
		a.src = l == 0 ? src : pp[(l - 1) & 1];
		a.src_ls = l == 0 ? ls : pitch;
		a.src_es = l == 0 ? es : 4;
		a.n_lines = n_lines;
		a.N = N;
		a.level = level0 + l;
		a.out_l = last ? nullptr : pp[l & 1];
		a.l_ls = pitch;
		a.l_es = 4;
		a.out_l2 = l_mode == 2 ? dst_l + (long)l * plane_stride : l_mode == 1 && last ? dst_l : nullptr;
		a.l2_ls = dls;
		a.l2_es = l_es;
		a.out_h = dst_h ? dst_h + (long)l * plane_stride : nullptr; // (null: the level passes of an L-only caller)
		a.h_ls = dls;
		a.h_es = h_es;
		a.border = border;
		if (launched(launch_swt_level(w, a, g.stream), "SWT", "level"))
			return 1;
	}
	return 0;
}

// Host or device memory (all sides alike); the checks of the C-ABI entries.
int swt1d(int wavelet, const void *src, long ls, long es, int n_lines, int N, int level0, int levels, void *dst_h, long h_es, void *dst_l,
	long l_es, int l_mode, long plane_stride, long dls, int border)
{
	Wavelet w;
	if (!wavelet_of(wavelet, &w) || (w != kCdf97S && w != kCdf53S))
		return fail("the SWT takes DWT_HIP_CDF97_S or DWT_HIP_CDF53_S (got wavelet %d)", wavelet);
	if (border != DWT_HIP_SWT_BORDER_REPLICATE && border != DWT_HIP_SWT_BORDER_SYMMETRIC)
		return fail("SWT: border %d (0: replicated, 1: symmetric)", border);
	if (n_lines < 0 || N < 0 || levels < 0 || level0 < 0 || level0 + (long)levels > SWT_MAX_LEVELS)
		return fail("SWT: bad arguments (%d lines of %d samples, levels %d .. %ld; at most %d levels)", n_lines, N, level0,
			level0 + (long)levels, SWT_MAX_LEVELS);
	if (l_mode < 0 || l_mode > 2)
		return fail("SWT: l_mode %d (0: no L, 1: the last level's, 2: every level's)", l_mode);
	if (n_lines == 0 || N == 0 || levels == 0)
		return 0;
	if (!src || !dst_h || (l_mode && !dst_l))
		return fail("null pointer argument");
	if (es < 4 || h_es < 4 || (l_mode && l_es < 4) || ls < 0 || dls < 0 || plane_stride < 0)
		return fail("SWT: bad strides");
	if (n_lines > 1 && (ls < es * (long)N || dls < h_es * (long)N || (l_mode && dls < l_es * (long)N)))
		return fail("SWT: lines must be apart (line strides %ld and %ld bytes, %d samples)", ls, dls, N);
	const long rows_bytes = (n_lines - 1l) * dls;
	if (levels > 1 && plane_stride < rows_bytes + h_es * (long)N)
		return fail("SWT: planes must be apart (plane stride %ld bytes)", plane_stride);
	// extents in bytes; src must not overlap an output, nor the outputs each other
	const size_t src_n = (size_t)((n_lines - 1l) * ls + (N - 1l) * es + 4);
	const size_t h_n = (size_t)((levels - 1l) * plane_stride + rows_bytes + (N - 1l) * h_es + 4);
	const size_t l_n = !l_mode ? 0 : (size_t)((l_mode == 2 ? (levels - 1l) * plane_stride : 0) + rows_bytes + (N - 1l) * l_es + 4);
	if (overlap(src, src_n, dst_h, h_n) || overlap(src, src_n, dst_l, l_n) || overlap(dst_h, h_n, dst_l, l_n))
		return fail("SWT: src, dst_h and dst_l must not overlap");
	if (check_inited())
		return 1;
	const bool dev = dwt_hip_is_device_pointer(src);
	if (dev != (bool)dwt_hip_is_device_pointer(dst_h) || (l_mode && dev != (bool)dwt_hip_is_device_pointer(dst_l)))
		return fail("src, dst_h and dst_l must all be host or all be device pointers");
	if (dev)
		return swt_device(w, (const char *)src, ls, es, n_lines, N, level0, levels, (char *)dst_h, h_es, (char *)dst_l, l_es, l_mode,
			plane_stride, dls, border);

	// host memory: a dense device image of the lines, dense device planes, each plane spread back
	const Frame fs{(void *)src, ls, es, 4, N, n_lines, false}, fh{dst_h, dls, h_es, 4, N, n_lines, false}, fl{dst_l, dls, l_es, 4, N, n_lines, false};
	if (frame_check(fs) || frame_check(fh) || frame_check(fl))
		return 1;
	const long pitch = frame_pitch(4, N), plane = pitch * n_lines;
	const int l_planes = l_mode == 2 ? levels : l_mode;
	Img A;
	if (grow(g.frame_b, (size_t)plane * (levels + l_planes)) || frame_stage(fs, g.frame_a, &A))
		return 1;
	char *dh = (char *)g.frame_b.p, *dl = dh + (size_t)plane * levels;
	if (swt_device(w, A.p, pitch, 4, n_lines, N, level0, levels, dh, 4, dl, 4, l_mode, plane, pitch, border))
		return 1;
	return frame_unpack_stack(fh, levels, plane_stride, dh, pitch) || frame_unpack_stack(fl, l_planes, plane_stride, dl, pitch);
}

} // namespace dwtb

using namespace dwtb;

#pragma GCC visibility push(default)
extern "C" {

int dwt_hip_swt1d_batch_ex(int wavelet, const void *src, size_t line_stride, size_t elem_stride, int n_lines, int N, int levels, void *dst_h,
	void *dst_l, int l_mode, size_t plane_stride, size_t dst_line_stride, int border)
{
	if (line_stride > (size_t)LONG_MAX / 2 || elem_stride > INT_MAX || plane_stride > (size_t)LONG_MAX / 64 || dst_line_stride > (size_t)LONG_MAX / 2)
		return fail("SWT: bad strides");
	return swt1d(wavelet, src, (long)line_stride, (long)elem_stride, n_lines, N, 0, levels, dst_h, 4, dst_l, 4, l_mode, (long)plane_stride,
		(long)dst_line_stride, border);
}

int dwt_hip_swt1d_batch(int wavelet, const void *src, size_t line_stride, size_t elem_stride, int n_lines, int N, int levels, void *dst_h,
	void *dst_l, int l_mode, size_t plane_stride, size_t dst_line_stride)
{
	return dwt_hip_swt1d_batch_ex(wavelet, src, line_stride, elem_stride, n_lines, N, levels, dst_h, dst_l, l_mode, plane_stride, dst_line_stride,
		DWT_HIP_SWT_BORDER_REPLICATE);
}

int dwt_hip_swt1d_level(int wavelet, const void *src, void *dst_l, void *dst_h, int N, int stride, int level)
{
	if (stride < 4)
		return fail("SWT: stride %d bytes", stride);
	if (N < 0 || level < 0 || level >= SWT_MAX_LEVELS)
		return fail("SWT: bad arguments (%d samples, level %d; levels 0 .. %d)", N, level, SWT_MAX_LEVELS - 1);
	const long line = (long)N * stride;
	return swt1d(wavelet, src, line, stride, 1, N, level, 1, dst_h, stride, dst_l, stride, 1, line, line, DWT_HIP_SWT_BORDER_REPLICATE);
}

} // extern "C"
#pragma GCC visibility pop
