// dwt_backend_iswt.hip -- the inverse stationary wavelet transforms of row batches and image batches under the symmetric
// border, and their C-ABI (include/libdwt_hip.h).
//
// Rows: dense device lines of up to N1D_MAX samples run every level in ONE launch of k_iswt_lines (dwt_iswt1d.hip).  Longer
// lines, strided destination elements and every call under option "swt_fused" = 0 run one k_iswt_level launch per level,
// the L chain ping-ponged through library scratch.  Images: a level below ISWT2D_FUSED_LEVELS with a dense destination is
// ONE launch of k_iswt2d_fused (dwt_iswt2d.hip) for the whole batch; deeper levels, a strided destination (level 0 only:
// every other level writes library scratch) and every call under option "swt2d_fused" = 0 take a column-pass launch and a
// row-pass launch, Lr and Hr in library scratch.  The LL chain ping-pongs through library scratch.  Host memory takes
// the staging detour (dwt_backend.h).  The operator tables are host memory and travel as kernel arguments.
#include "dwt_backend.h"

#include <climits>

namespace dwtb {

namespace {

int iswt_wavelet(int wavelet, int border, Wavelet *w)
{
	if (!wavelet_of(wavelet, w) || (*w != kCdf97S && *w != kCdf53S))
		return fail("the inverse SWT takes DWT_HIP_CDF97_S or DWT_HIP_CDF53_S (got wavelet %d)", wavelet);
	if (border == DWT_HIP_SWT_BORDER_REPLICATE)
		return fail("inverse SWT: replicated borders do not reconstruct; transform and invert under DWT_HIP_SWT_BORDER_SYMMETRIC");
	if (border != DWT_HIP_SWT_BORDER_SYMMETRIC)
		return fail("inverse SWT: border %d (1: symmetric)", border);
	return 0;
}

// the caller's tables of n entries -> op[], prm[] (NULL tables: KEEP everywhere)
int iswt_tables(const int *ops, const float *params, int n, int *op, float *prm)
{
	for (int i = 0; i < n; i++) {
		op[i] = ops ? ops[i] : (int)kBandKeep;
		prm[i] = params ? params[i] : 0.f;
		if (op[i] == DWT_HIP_BAND_COMPRESS)
			return fail("inverse SWT: DWT_HIP_BAND_COMPRESS is not an operator on load (plane %d); apply it to the stored plane", i);
		if (op[i] < DWT_HIP_BAND_KEEP || op[i] > DWT_HIP_BAND_SOFT)
			return fail("inverse SWT: operator %d of plane %d (DWT_HIP_BAND_KEEP .. _SOFT)", op[i], i);
		if (!params && op[i] != DWT_HIP_BAND_KEEP && op[i] != DWT_HIP_BAND_ZERO)
			return fail("inverse SWT: operator %d of plane %d needs a parameter table", op[i], i);
	}
	return 0;
}

// ---- rows: device memory on every side ----
int iswt1d_device(Wavelet w, const char *src_h, const char *src_l, long ps, long sls, int n_lines, int N, int levels, const int *op,
	const float *prm, char *dst, long dls, long des)
{
	if (check_dev_align({levels ? src_h : nullptr, src_l, dst}, {levels > 1 ? ps : 0, sls, dls, des}))
		return 1;
	if (levels == 0)
		return frame_unpack(Frame{dst, dls, des, 4, N, n_lines, true}, src_l, sls);
	if (g.swt_fused && N <= N1D_MAX && des == 4) {
		IswtLineArgs a{};
		a.src_h = src_h;
		a.src_l = src_l;
		a.plane_stride = ps;
		a.src_line_stride = sls;
		a.n_lines = n_lines;
		a.N = N;
		a.levels = levels;
		a.vec = all16({(uintptr_t)src_h, (uintptr_t)src_l, (uintptr_t)(levels > 1 ? ps : 0), (uintptr_t)sls});
		for (int l = 0; l < levels; l++)
			a.op[l] = op[l], a.param[l] = prm[l];
		a.dst = dst;
		a.dst_line_stride = dls;
		return launched(launch_iswt_lines(w, a, g.stream), "inverse SWT", "line");
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
	for (int l = levels - 1, s = 0; l >= 0; l--, s++) {
		IswtLevelArgs a{};
		a.src_l = s == 0 ? src_l : pp[(s - 1) & 1];
		a.l_ls = s == 0 ? sls : pitch;
		a.src_h = src_h + (long)l * ps;
		a.h_ls = sls;
		a.n_lines = n_lines;
		a.N = N;
		a.level = l;
		a.op = op[l];
		a.param = prm[l];
		a.dst = l == 0 ? dst : pp[s & 1];
		a.d_ls = l == 0 ? dls : pitch;
		a.d_es = l == 0 ? des : 4;
		if (launched(launch_iswt_level(w, a, g.stream), "inverse SWT", "level"))
			return 1;
	}
	return 0;
}

int iswt1d(int wavelet, int border, const void *src_h, const void *src_l, long ps, long sls, int n_lines, int N, int levels, const int *ops,
	const float *params, void *dst, long dls, long des)
{
	Wavelet w;
	if (iswt_wavelet(wavelet, border, &w))
		return 1;
	if (n_lines < 0 || N < 0 || levels < 0 || levels > SWT_MAX_LEVELS)
		return fail("inverse SWT: bad arguments (%d lines of %d samples, %d levels; at most %d levels)", n_lines, N, levels, SWT_MAX_LEVELS);
	int op[SWT_MAX_LEVELS];
	float prm[SWT_MAX_LEVELS];
	if (iswt_tables(ops, params, levels, op, prm))
		return 1;
	if (n_lines == 0 || N == 0)
		return 0;
	if (!src_l || !dst || (levels && !src_h))
		return fail("null pointer argument");
	if (des < 4 || sls < 0 || dls < 0 || ps < 0)
		return fail("inverse SWT: bad strides");
	if (n_lines > 1 && (sls < 4l * N || dls < des * (long)N))
		return fail("inverse SWT: lines must be apart (line strides %ld and %ld bytes, %d samples)", sls, dls, N);
	const long rows_bytes = (n_lines - 1l) * sls;
	if (levels > 1 && ps < rows_bytes + 4l * N)
		return fail("inverse SWT: planes must be apart (plane stride %ld bytes)", ps);
	const size_t l_n = (size_t)(rows_bytes + 4l * N), h_n = levels ? (size_t)((levels - 1l) * ps + rows_bytes + 4l * N) : 0;
	const size_t d_n = (size_t)((n_lines - 1l) * dls + (N - 1l) * des + 4);
	if (overlap(dst, d_n, src_h, h_n) || overlap(dst, d_n, src_l, l_n))
		return fail("inverse SWT: dst must not overlap src_h or src_l");
	if (check_inited())
		return 1;
	const bool dev = dwt_hip_is_device_pointer(dst);
	if (dev != (bool)dwt_hip_is_device_pointer(src_l) || (levels && dev != (bool)dwt_hip_is_device_pointer(src_h)))
		return fail("src_h, src_l and dst must all be host or all be device pointers");
	if (dev)
		return iswt1d_device(w, (const char *)src_h, (const char *)src_l, ps, sls, n_lines, N, levels, op, prm, (char *)dst, dls, des);

	// host memory: dense device planes of the sources (a ZERO plane does not cross), a dense device image of the result
	const Frame fh{(void *)src_h, sls, 4, 4, N, n_lines, false}, fl{(void *)src_l, sls, 4, 4, N, n_lines, false}, fd{dst, dls, des, 4, N, n_lines, false};
	if (frame_check(fh) || frame_check(fd))
		return 1;
	const long pitch = frame_pitch(4, N), plane = pitch * n_lines;
	if (grow(g.frame_b, (size_t)plane * (levels + 2)))
		return 1;
	char *const dh = (char *)g.frame_b.p, *const dl = dh + (size_t)plane * levels, *const dd = dl + plane;
	for (int l = 0; l < levels; l++) {
		Frame f = fh;
		f.p = (char *)src_h + (size_t)l * ps;
		if (op[l] != kBandZero && frame_pack(f, dh + (size_t)plane * l, pitch))
			return 1;
	}
	if (frame_pack(fl, dl, pitch) || iswt1d_device(w, dh, dl, plane, pitch, n_lines, N, levels, op, prm, dd, pitch, 4))
		return 1;
	return frame_unpack(fd, dd, pitch);
}

// ---- images: device memory on every side ----
bool level_fused(const Iswt2dLevelArgs &a) { return g.swt2d_fused && iswt2d_fused_fits(a); }

// detail band k of level l of image b at src_h + b*sbs + (3*l + k-1)*ps, rows ssx bytes apart, dense; the last level's LL of
// image b at src_l + b*sbs
int iswt2d_device(Wavelet w, const char *src_h, const char *src_l, long sbs, long ps, long ssx, int batch, int W, int H, int levels,
	const int *op, const float *prm, char *dst, long dbs, long dsx, long dsy)
{
	if (check_dev_align({levels ? src_h : nullptr, src_l, dst}, {batch > 1 ? sbs : 0, levels ? ps : 0, ssx, batch > 1 ? dbs : 0, dsx, dsy}))
		return 1;
	if (levels == 0) {
		for (int b = 0; b < batch; b++)
			if (frame_unpack(Frame{dst + (size_t)b * dbs, dsx, dsy, 4, W, H, true}, src_l + (size_t)b * sbs, ssx))
				return 1;
		return 0;
	}
	const size_t img = (size_t)4 * W * H * batch; // one dense scratch plane of the whole batch
	const bool chain = levels > 1;
	bool passes = false; // does any level take the two passes?
	for (int l = 0; l < levels; l++) {
		Iswt2dLevelArgs probe{};
		probe.dst_sy = l ? 4 : dsy; // (level 0 writes the caller's elements; every other level writes dense planes)
		probe.H = H;
		probe.batch = batch;
		probe.level = l;
		passes = passes || !level_fused(probe);
	}
	if ((chain || passes) && grow(g.swt_ws, img * ((chain ? 2 : 0) + (passes ? 2 : 0))))
		return 1;
	char *const ws = (char *)g.swt_ws.p;
	char *const pp[2] = {ws, ws + img}, *const pass_ws = ws + (chain ? 2 * img : 0);
	for (int l = levels - 1, s = 0; l >= 0; l--, s++) {
		Iswt2dLevelArgs a{};
		a.W = W;
		a.H = H;
		a.batch = batch;
		a.level = l;
		if (s == 0)
			a.ll = src_l, a.ll_bs = sbs, a.ll_sx = ssx;
		else
			a.ll = pp[(s - 1) & 1], a.ll_bs = 4l * W * H, a.ll_sx = 4l * W;
		a.hl = src_h + (3l * l + 0) * ps;
		a.lh = src_h + (3l * l + 1) * ps;
		a.hh = src_h + (3l * l + 2) * ps;
		a.d_bs = sbs;
		a.d_sx = ssx;
		for (int k = 0; k < 3; k++)
			a.op[k] = op[3 * l + k], a.param[k] = prm[3 * l + k];
		if (l == 0)
			a.dst = dst, a.dst_bs = dbs, a.dst_sx = dsx, a.dst_sy = dsy;
		else
			a.dst = pp[s & 1], a.dst_bs = 4l * W * H, a.dst_sx = 4l * W, a.dst_sy = 4;
		if (level_fused(a)) {
			if (launched(launch_iswt2d_fused(w, a, g.stream), "inverse SWT 2-D", "fused level"))
				return 1;
			continue;
		}
		a.lr = pass_ws;
		a.hr = pass_ws + img;
		if (launched(launch_iswt2d_cols(w, a, g.stream), "inverse SWT 2-D", "column pass") ||
			launched(launch_iswt2d_rows(w, a, g.stream), "inverse SWT 2-D", "row pass"))
			return 1;
	}
	return 0;
}

int iswt2d(int wavelet, int border, const void *src_h, const void *src_l, long sbs, long ps, long ssx, int batch, int W, int H, int levels,
	const int *ops, const float *params, void *dst, long dbs, long dsx, long dsy)
{
	Wavelet w;
	if (iswt_wavelet(wavelet, border, &w))
		return 1;
	if (batch < 1 || W < 1 || H < 1 || levels < 0 || levels > SWT_MAX_LEVELS)
		return fail("inverse SWT 2-D: bad arguments (%d images of %d x %d, %d levels; at least one image and sample, at most %d levels)", batch, W,
			H, levels, SWT_MAX_LEVELS);
	int op[3 * SWT_MAX_LEVELS];
	float prm[3 * SWT_MAX_LEVELS];
	if (iswt_tables(ops, params, 3 * levels, op, prm))
		return 1;
	if (!src_l || !dst || (levels && !src_h))
		return fail("null pointer argument");
	if (dsy < 4 || ssx < 4l * W || dsx < dsy * (long)W)
		return fail("inverse SWT 2-D: bad strides (rows %ld and %ld bytes apart, dst elements %ld; %d samples a row)", ssx, dsx, dsy, W);
	const long plane = (H - 1l) * ssx + 4l * W; // bytes a source plane occupies
	if (levels && ps < plane)
		return fail("inverse SWT 2-D: planes must be apart (plane stride %ld bytes, a plane takes %ld)", ps, plane);
	const size_t h_1 = levels ? (size_t)((3l * levels - 1) * ps + plane) : 0, l_1 = (size_t)plane,
		     d_1 = (size_t)((H - 1l) * dsx + (W - 1l) * dsy + 4);
	if (batch > 1 && ((size_t)sbs < h_1 || (size_t)sbs < l_1 || (size_t)dbs < d_1))
		return fail("inverse SWT 2-D: images must be apart (batch strides %ld and %ld bytes)", sbs, dbs);
	const size_t h_n = levels ? (size_t)(batch - 1l) * sbs + h_1 : 0, l_n = (size_t)(batch - 1l) * sbs + l_1, d_n = (size_t)(batch - 1l) * dbs + d_1;
	if (overlap(dst, d_n, src_h, h_n) || overlap(dst, d_n, src_l, l_n))
		return fail("inverse SWT 2-D: dst must not overlap src_h or src_l");
	if (check_inited())
		return 1;
	const bool dev = dwt_hip_is_device_pointer(dst);
	if (dev != (bool)dwt_hip_is_device_pointer(src_l) || (levels && dev != (bool)dwt_hip_is_device_pointer(src_h)))
		return fail("src_h, src_l and dst must all be host or all be device pointers");
	if (dev)
		return iswt2d_device(w, (const char *)src_h, (const char *)src_l, sbs, ps, ssx, batch, W, H, levels, op, prm, (char *)dst, dbs, dsx, dsy);

	// host memory: dense device planes of the sources (a ZERO plane does not cross), dense device images of the result
	const Frame fs{nullptr, ssx, 4, 4, W, H, false}, fd{nullptr, dsx, dsy, 4, W, H, false};
	if (frame_check(fs) || frame_check(fd))
		return 1;
	const long pitch = frame_pitch(4, W), dplane = pitch * H;
	// image b: its 3 * levels detail planes and its LL behind them (src_h and src_l share the batch stride); then the results
	const size_t per = (size_t)dplane * (3 * levels + 1);
	if (grow(g.frame_b, per * batch + (size_t)dplane * batch))
		return 1;
	char *const dh = (char *)g.frame_b.p, *const dl = dh + (size_t)dplane * 3 * levels, *const dd = dh + per * batch;
	for (int b = 0; b < batch; b++) {
		Frame f = fs;
		for (int k = 0; k < 3 * levels; k++) {
			f.p = (char *)src_h + (size_t)b * sbs + (size_t)k * ps;
			if (op[k] != kBandZero && frame_pack(f, dh + b * per + (size_t)k * dplane, pitch))
				return 1;
		}
		f.p = (char *)src_l + (size_t)b * sbs;
		if (frame_pack(f, dl + b * per, pitch))
			return 1;
	}
	if (iswt2d_device(w, dh, dl, (long)per, dplane, pitch, batch, W, H, levels, op, prm, dd, dplane, pitch, 4))
		return 1;
	for (int b = 0; b < batch; b++) {
		Frame f = fd;
		f.p = (char *)dst + (size_t)b * dbs;
		if (frame_unpack(f, dd + (size_t)b * dplane, pitch))
			return 1;
	}
	return 0;
}

} // namespace

} // namespace dwtb

using namespace dwtb;

#pragma GCC visibility push(default)
extern "C" {

int dwt_hip_iswt1d_batch(int wavelet, int border, const void *src_h, const void *src_l, size_t plane_stride, size_t src_line_stride, int n_lines,
	int N, int levels, const int *ops, const float *params, void *dst, size_t dst_line_stride, size_t dst_elem_stride)
{
	if (src_line_stride > (size_t)LONG_MAX / 2 || dst_elem_stride > INT_MAX || plane_stride > (size_t)LONG_MAX / 64 || dst_line_stride > (size_t)LONG_MAX / 2)
		return fail("inverse SWT: bad strides");
	return iswt1d(wavelet, border, src_h, src_l, (long)plane_stride, (long)src_line_stride, n_lines, N, levels, ops, params, dst,
		(long)dst_line_stride, (long)dst_elem_stride);
}

int dwt_hip_iswt2d_batch(int wavelet, int border, const void *src_h, const void *src_l, size_t src_batch_stride, size_t plane_stride,
	int src_stride_x, int batch, int size_x, int size_y, int levels, const int *ops, const float *params, void *dst, size_t dst_batch_stride,
	int dst_stride_x, int dst_stride_y)
{
	if (src_batch_stride > (size_t)LONG_MAX / 2 || dst_batch_stride > (size_t)LONG_MAX / 2 || plane_stride > (size_t)LONG_MAX / 128 || src_stride_x < 0 ||
		dst_stride_x < 0 || dst_stride_y < 0)
		return fail("inverse SWT 2-D: bad strides");
	return iswt2d(wavelet, border, src_h, src_l, (long)src_batch_stride, (long)plane_stride, src_stride_x, batch, size_x, size_y, levels, ops,
		params, dst, (long)dst_batch_stride, dst_stride_x, dst_stride_y);
}

} // extern "C"
#pragma GCC visibility pop
