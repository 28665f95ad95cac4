// dwt_backend_swt2d.hip -- the stationary wavelet transform of image batches on the device, and its C-ABI
// (include/libdwt_hip.h).
//
// A level of dense device images below SWT2D_FUSED_LEVELS is ONE launch of k_swt2d_fused (dwt_swt2d.hip) for the whole
// batch.  Strided elements, deeper levels and every call under option "swt2d_fused" = 0 take the generic route: a row-pass
// launch and a column-pass launch per level, Lr and Hr in library scratch.  The LL chain runs through the caller's LL
// planes (l_mode 2) or ping-pongs through library scratch.  Host memory takes the staging detour (dwt_backend.h).
#include "dwt_backend.h"

#include <climits>

namespace dwtb {

namespace {

bool level_fused(const Swt2dLevelArgs &a) { return g.swt2d_fused && swt2d_fused_fits(a); }

// one level, device memory on every side; a.lr / a.hr are filled in here when the passes run
int swt2d_level_device(Wavelet w, Swt2dLevelArgs a, char *passes)
{
	if (level_fused(a))
		return launched(launch_swt2d_fused(w, a, g.stream), "SWT 2-D", "fused level");
	a.lr = passes;
	a.hr = passes + (size_t)4 * a.W * a.H * a.batch;
	return launched(launch_swt2d_rows(w, a, g.stream), "SWT 2-D", "row pass") || launched(launch_swt2d_cols(w, a, g.stream), "SWT 2-D", "column pass");
}

// Every level of a batch in device memory.  Detail band k of level l of image b at dst_h + b*h_bs + (3*l + k-1)*ps, rows
// dsx bytes apart, dense; LL by l_mode at dst_l + b*l_bs (+ l*ps).  Source elements sy bytes apart.
int swt2d_device(Wavelet w, const char *src, long sbs, long sx, long sy, int batch, int W, int H, int levels, char *dst_h, long h_bs,
	char *dst_l, long l_bs, int l_mode, long ps, long dsx, int border)
{
	if (check_dev_align({src, dst_h, l_mode ? dst_l : nullptr}, {sbs, sx, sy, h_bs, l_mode ? l_bs : 0, ps, dsx}))
		return 1;
	const size_t img = (size_t)4 * W * H * batch; // one dense scratch plane of the whole batch
	const bool chain = l_mode != 2 && levels > 1;
	bool passes = false; // does any level take the two passes?
	for (int l = 0; l < levels; l++) {
		Swt2dLevelArgs probe{};
		probe.src_sy = l ? 4 : sy; // (level 0 reads the caller's elements; every later level reads dense planes)
		probe.d_sy = 4;
		probe.H = H;
		probe.batch = batch;
		probe.level = l;
		passes = passes || !level_fused(probe);
	}
	if ((chain || passes) && grow(g.swt_ws, img * ((chain ? 2 : 0) + (passes ? 2 : 0))))
		return 1;
	char *const ws = (char *)g.swt_ws.p;
	char *const pp[2] = {ws, ws + img}, *const pass_ws = ws + (chain ? 2 * img : 0);
	for (int l = 0; l < levels; l++) {
		const bool last = l == levels - 1;
		Swt2dLevelArgs a{};
		a.W = W;
		a.H = H;
		a.batch = batch;
		a.level = l;
		if (l == 0) {
			a.src = src, a.src_bs = sbs, a.src_sx = sx, a.src_sy = sy;
		} else if (l_mode == 2) {
			a.src = dst_l + (long)(l - 1) * ps, a.src_bs = l_bs, a.src_sx = dsx, a.src_sy = 4;
		} else {
			a.src = pp[(l - 1) & 1], a.src_bs = 4l * W * H, a.src_sx = 4l * W, a.src_sy = 4;
		}
		if (l_mode == 2 || (l_mode == 1 && last)) {
			a.ll = dst_l + (l_mode == 2 ? (long)l * ps : 0), a.ll_bs = l_bs, a.ll_sx = dsx;
		} else if (!last) {
			a.ll = pp[l & 1], a.ll_bs = 4l * W * H, a.ll_sx = 4l * W;
		}
		a.hl = dst_h + (3l * l + 0) * ps;
		a.lh = dst_h + (3l * l + 1) * ps;
		a.hh = dst_h + (3l * l + 2) * ps;
		a.d_bs = h_bs;
		a.d_sx = dsx;
		a.d_sy = 4;
		a.border = border;
		if (swt2d_level_device(w, a, pass_ws))
			return 1;
	}
	return 0;
}

int swt2d_wavelet(int wavelet, Wavelet *w)
{
	if (!wavelet_of(wavelet, w) || (*w != kCdf97S && *w != kCdf53S))
		return fail("the SWT takes DWT_HIP_CDF97_S or DWT_HIP_CDF53_S (got wavelet %d)", wavelet);
	return 0;
}

// bytes from the first to the last byte of a w x h frame
size_t frame_extent(long sx, long sy, int w, int h) { return (size_t)((h - 1l) * sx + (w - 1l) * sy + 4); }

int swt2d_batch(int wavelet, const void *src, long sbs, int batch, long sx, long sy, int W, int H, int levels, void *dst_h, void *dst_l,
	int l_mode, long dbs, long ps, long dsx, int border)
{
	Wavelet w;
	if (swt2d_wavelet(wavelet, &w))
		return 1;
	if (border != DWT_HIP_SWT_BORDER_REPLICATE && border != DWT_HIP_SWT_BORDER_SYMMETRIC)
		return fail("SWT 2-D: border %d (0: replicated, 1: symmetric)", border);
	if (batch < 1 || W < 1 || H < 1 || levels < 0 || levels > SWT_MAX_LEVELS)
		return fail("SWT 2-D: bad arguments (%d images of %d x %d, %d levels; at least one image and sample, at most %d levels)", batch, W, H,
			levels, SWT_MAX_LEVELS);
	if (l_mode < 0 || l_mode > 2)
		return fail("SWT 2-D: l_mode %d (0: no LL, 1: the last level's, 2: every level's)", l_mode);
	if (levels == 0)
		return 0;
	if (!src || !dst_h || (l_mode && !dst_l))
		return fail("null pointer argument");
	if (sy < 4 || sx < sy * (long)W || dsx < 4l * W)
		return fail("SWT 2-D: bad strides (rows %ld and %ld bytes apart, elements %ld; %d samples a row)", sx, dsx, sy, W);
	const long plane = (H - 1l) * dsx + 4l * W; // bytes a plane occupies
	if (ps < plane)
		return fail("SWT 2-D: planes must be apart (plane stride %ld bytes, a plane takes %ld)", ps, plane);
	const int l_planes = l_mode == 2 ? levels : l_mode;
	const size_t src_1 = frame_extent(sx, sy, W, H), h_1 = (size_t)((3l * levels - 1) * ps + plane),
		     l_1 = l_planes ? (size_t)((l_planes - 1l) * ps + plane) : 0;
	if (batch > 1 && ((size_t)sbs < src_1 || (size_t)dbs < h_1 || (size_t)dbs < l_1))
		return fail("SWT 2-D: images must be apart (batch strides %ld and %ld bytes)", sbs, dbs);
	const size_t src_n = (size_t)(batch - 1l) * sbs + src_1, h_n = (size_t)(batch - 1l) * dbs + h_1, l_n = l_planes ? (size_t)(batch - 1l) * dbs + l_1 : 0;
	// dst_h and dst_l share the batch stride, so their images may interleave (every image's LL planes behind its detail
	// planes): inside the common range image b of dst_l lies d bytes behind the start of some image of dst_h
	bool hl = overlap(dst_h, h_n, dst_l, l_n);
	if (hl && batch > 1) {
		const long d = (long)(((intptr_t)dst_l - (intptr_t)dst_h) % dbs + dbs) % dbs;
		hl = (size_t)d < h_1 || (size_t)d + l_1 > (size_t)dbs;
	}
	if (overlap(src, src_n, dst_h, h_n) || overlap(src, src_n, dst_l, l_n) || hl)
		return fail("SWT 2-D: src, dst_h and dst_l must not overlap");
	if (check_inited())
		return 1;
	const bool dev = dwt_hip_is_device_pointer(src);
	if (dev != (bool)dwt_hip_is_device_pointer(dst_h) || (l_mode && dev != (bool)dwt_hip_is_device_pointer(dst_l)))
		return fail("src, dst_h and dst_l must all be host or all be device pointers");
	if (dev)
		return swt2d_device(w, (const char *)src, sbs, sx, sy, batch, W, H, levels, (char *)dst_h, dbs, (char *)dst_l, dbs, l_mode, ps, dsx, border);

	// host memory: dense device images of the batch, dense device planes, each plane spread back
	const Frame fs{(void *)src, sx, sy, 4, W, H, false}, fh{dst_h, dsx, 4, 4, W, H, false}, fl{dst_l, dsx, 4, 4, W, H, false};
	if (frame_check(fs) || frame_check(fh))
		return 1;
	const long pitch = frame_pitch(4, W), dplane = pitch * H;
	if (grow(g.frame_a, (size_t)dplane * batch) || grow(g.frame_b, (size_t)dplane * batch * (3 * levels + l_planes)))
		return 1;
	char *const ds = (char *)g.frame_a.p, *const dh = (char *)g.frame_b.p, *const dl = dh + (size_t)dplane * batch * 3 * levels;
	if (frame_pack_stack(fs, batch, sbs, ds, pitch))
		return 1;
	if (swt2d_device(w, ds, dplane, pitch, 4, batch, W, H, levels, dh, dplane * 3 * levels, dl, dplane * l_planes, l_mode, dplane, pitch, border))
		return 1;
	for (int b = 0; b < batch; b++) {
		Frame h = fh, l = fl;
		h.p = (char *)dst_h + (size_t)b * dbs;
		l.p = l_planes ? (char *)dst_l + (size_t)b * dbs : nullptr;
		if (frame_unpack_stack(h, 3 * levels, ps, dh + (size_t)b * dplane * 3 * levels, pitch) ||
			frame_unpack_stack(l, l_planes, ps, dl + (size_t)b * dplane * l_planes, pitch))
			return 1;
	}
	return 0;
}

int swt2d_level(int wavelet, const void *src, long sx, long sy, int W, int H, int level, void *const dst[4], long dsx, long dsy)
{
	Wavelet w;
	if (swt2d_wavelet(wavelet, &w))
		return 1;
	if (W < 1 || H < 1 || level < 0 || level >= SWT_MAX_LEVELS)
		return fail("SWT 2-D: bad arguments (%d x %d samples, level %d; levels 0 .. %d)", W, H, level, SWT_MAX_LEVELS - 1);
	if (!src || !dst[0] || !dst[1] || !dst[2] || !dst[3])
		return fail("null pointer argument");
	if (sy < 4 || dsy < 4 || sx < sy * (long)W || dsx < dsy * (long)W)
		return fail("SWT 2-D: bad strides (rows %ld and %ld bytes apart, elements %ld and %ld; %d samples a row)", sx, dsx, sy, dsy, W);
	const size_t src_n = frame_extent(sx, sy, W, H), dst_n = frame_extent(dsx, dsy, W, H);
	for (int i = 0; i < 4; i++) {
		if (overlap(src, src_n, dst[i], dst_n))
			return fail("SWT 2-D: src and the four planes must not overlap");
		for (int k = 0; k < i; k++)
			if (overlap(dst[k], dst_n, dst[i], dst_n))
				return fail("SWT 2-D: src and the four planes must not overlap");
	}
	if (check_inited())
		return 1;
	const bool dev = dwt_hip_is_device_pointer(src);
	for (int i = 0; i < 4; i++)
		if (dev != (bool)dwt_hip_is_device_pointer(dst[i]))
			return fail("src and the four planes must all be host or all be device pointers");
	Swt2dLevelArgs a{};
	a.W = W;
	a.H = H;
	a.batch = 1;
	a.level = level;
	const Frame fs{(void *)src, sx, sy, 4, W, H, false};
	const long pitch = frame_pitch(4, W), dplane = pitch * H;
	if (dev) {
		if (check_dev_align({src, dst[0], dst[1], dst[2], dst[3]}, {sx, sy, dsx, dsy}))
			return 1;
		a.src = (const char *)src, a.src_sx = sx, a.src_sy = sy;
		a.ll = (char *)dst[0], a.hl = (char *)dst[1], a.lh = (char *)dst[2], a.hh = (char *)dst[3];
		a.ll_sx = a.d_sx = dsx;
		a.d_sy = dsy;
	} else {
		Frame fd{nullptr, dsx, dsy, 4, W, H, false};
		Img A;
		if (frame_check(fs) || frame_check(fd) || grow(g.frame_b, (size_t)4 * dplane) || frame_stage(fs, g.frame_a, &A))
			return 1;
		char *const d = (char *)g.frame_b.p;
		a.src = A.p, a.src_sx = pitch, a.src_sy = 4;
		a.ll = d, a.hl = d + dplane, a.lh = d + 2 * dplane, a.hh = d + 3 * dplane;
		a.ll_sx = a.d_sx = pitch;
		a.d_sy = 4;
	}
	if (!level_fused(a) && grow(g.swt_ws, (size_t)8 * W * H))
		return 1;
	if (swt2d_level_device(w, a, (char *)g.swt_ws.p))
		return 1;
	if (dev)
		return 0;
	for (int i = 0; i < 4; i++) {
		const Frame fd{dst[i], dsx, dsy, 4, W, H, false};
		if (frame_unpack(fd, (char *)g.frame_b.p + (size_t)i * dplane, pitch))
			return 1;
	}
	return 0;
}

} // namespace

} // namespace dwtb

using namespace dwtb;

#pragma GCC visibility push(default)
extern "C" {

int dwt_hip_swt2d_batch_ex(int wavelet, const void *src, size_t batch_stride, int batch, int stride_x, int stride_y, int size_x, int size_y,
	int levels, void *dst_h, void *dst_l, int l_mode, size_t dst_batch_stride, size_t plane_stride, int dst_stride_x, int border)
{
	if (batch_stride > (size_t)LONG_MAX / 2 || dst_batch_stride > (size_t)LONG_MAX / 2 || plane_stride > (size_t)LONG_MAX / 128 || stride_x < 0 ||
		stride_y < 0 || dst_stride_x < 0)
		return fail("SWT 2-D: bad strides");
	return swt2d_batch(wavelet, src, (long)batch_stride, batch, stride_x, stride_y, size_x, size_y, levels, dst_h, dst_l, l_mode,
		(long)dst_batch_stride, (long)plane_stride, dst_stride_x, border);
}

int dwt_hip_swt2d_batch(int wavelet, const void *src, size_t batch_stride, int batch, int stride_x, int stride_y, int size_x, int size_y,
	int levels, void *dst_h, void *dst_l, int l_mode, size_t dst_batch_stride, size_t plane_stride, int dst_stride_x)
{
	return dwt_hip_swt2d_batch_ex(wavelet, src, batch_stride, batch, stride_x, stride_y, size_x, size_y, levels, dst_h, dst_l, l_mode,
		dst_batch_stride, plane_stride, dst_stride_x, DWT_HIP_SWT_BORDER_REPLICATE);
}

int dwt_hip_swt2d_level(int wavelet, const void *src, int stride_x, int stride_y, int size_x, int size_y, int level, void *dst_ll, void *dst_hl,
	void *dst_lh, void *dst_hh, int dst_stride_x, int dst_stride_y)
{
	void *const dst[4] = {dst_ll, dst_hl, dst_lh, dst_hh};
	return swt2d_level(wavelet, src, stride_x, stride_y, size_x, size_y, level, dst, dst_stride_x, dst_stride_y);
}

} // extern "C"
#pragma GCC visibility pop
