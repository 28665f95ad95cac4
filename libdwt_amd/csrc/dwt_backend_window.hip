// dwt_backend_window.hip -- windowed and reduced-resolution inverse 2-D transforms of dense Mallat frames and their C-ABI
// (include/libdwt_hip.h).
//
// A window [x0, x0 + w) x [y0, y0 + h) of LL(r) of every frame of a batch, bit for bit the crop of the full inverse of the
// frame's top-left Wo(r) x Ho(r) rectangle at J - r levels.  Two routes, option "window_fused":
//   0  the cross-check: the inverse driver (inverse2d) out of place into Ctx::win_ws, then a rectangle copy;
//   2  the window kernels (dwt_window2d.hip): one launch per level l = J .. r + 1 over the region of LL(l-1) that
//      dwt_hip_window_regions says the window needs; level J reads LL(J) from the frame, the levels between pass their
//      regions through two halves of Ctx::win_ws, the last level writes the caller's window;
//   1  (default) route 2 where it was measured to win (window_pays), else route 0.
// The level geometry travels in the kernels' arguments: no copy between host and device, no synchronisation, nothing
// allocated once win_ws has the shape's size.
#include "dwt_backend.h"

#include <climits>

namespace dwtb {

namespace {

static_assert(DWT_HIP_WINDOW_GRID_BATCH == WINDOW_GRID_BATCH && DWT_HIP_WINDOW_TILE == WINDOW_TILE, "the header states the kernels' constants");

struct WindowCall {
	Wavelet w;
	int es, J, r;
	int xywh[4 * DWT_HIP_BAND_MAX_SLOTS];
	// the region of LL(l) the window needs, l = r .. J: columns [x[l], x[l] + nx[l]), rows alike (l = r: the window itself)
	int x[33], nx[33], y[33], ny[33];
};

// The measured rule of route 1 (profiles/window_timing.json): the window kernels pay where the window covers
// at most 1 / 16 of LL(r) AND the cross-check route would move a band of 8192^2 samples or more over the batch.  Measured on
// one 8192^2 frame (float 9/7: 2.5x at 256^2, 2.0x at 512^2, 1.4x at 2048^2, 0.5x on the whole band) and on 16 frames of
// 4096^2 (5.4x at 512^2); on the 2048^2 band of discard 2 the inverse driver is three short launches and wins (0.5x).  Bands
// between 2048^2 and 8192^2 were not measured: they stay on the cross-check route.
constexpr long kWindowShareDen = 16;
constexpr long kWindowBandMin = 1l << 26;
bool window_pays(const WindowCall &c, int size_x, int size_y, int w, int h, int batch)
{
	const long Wr = ceil_div_pow2(size_x, c.r), Hr = ceil_div_pow2(size_y, c.r);
	return (long)w * h * kWindowShareDen <= Wr * Hr && Wr * Hr * batch >= kWindowBandMin;
}

int window_check(WindowCall *c, int wavelet, const void *src, size_t batch_stride, int batch, int stride_x, int size_x, int size_y, int j_max,
	int discard, int x0, int y0, int w, int h, const void *dst, size_t dst_batch_stride, int dst_stride_x)
{
	if (wavelet != DWT_HIP_CDF97_S && wavelet != DWT_HIP_CDF53_S && wavelet != DWT_HIP_INTERP53_S && wavelet != DWT_HIP_CDF53_I &&
	    wavelet != DWT_HIP_CDF53_I16)
		return fail("window: wavelet %d has no windowed inverse (DWT_HIP_CDF97_S, _CDF53_S, _INTERP53_S, _CDF53_I, _CDF53_I16)", wavelet);
	wavelet_of(wavelet, &c->w);
	c->es = elem_size(c->w);
	if (!src || !dst)
		return fail("null pointer argument");
	if (batch < 1 || batch > 65535)
		return fail("window: bad argument (batch must be 1..65535)");
	const int ns = dwt_hip_window_regions(wavelet, size_x, size_y, j_max, discard, x0, y0, w, h, c->xywh);
	if (ns < 0)
		return fail("window: bad sizes, level count or window (%d x %d, j_max %d, discard %d, window %d x %d at (%d, %d))", size_x, size_y, j_max,
			discard, w, h, x0, y0);
	c->J = (ns - 1) / 3, c->r = discard;
	const long es = c->es;
	if (stride_x < 0 || (stride_x % es) || stride_x < size_x * es || (batch_stride % es) || batch_stride < (size_t)stride_x * size_y ||
	    batch_stride > ((size_t)1 << 46) || (uintptr_t)src % es)
		return fail("window: bad strides of the source");
	if (dst_stride_x < 0 || (dst_stride_x % es) || dst_stride_x < w * es || (dst_batch_stride % es) || dst_batch_stride > ((size_t)1 << 46) ||
	    (uintptr_t)dst % es)
		return fail("window: bad strides of the destination");
	const size_t dst_frame = (size_t)(h - 1) * dst_stride_x + (size_t)w * es;
	if (batch > 1 && dst_batch_stride < dst_frame)
		return fail("window: the destination's frames must be apart (batch stride %zu bytes, a window takes %zu)", dst_batch_stride, dst_frame);
	const size_t dst_extent = (size_t)(batch - 1) * dst_batch_stride + dst_frame;
	const size_t src_frame = (size_t)(size_y - 1) * stride_x + (size_t)size_x * es;
	for (int b = 0; b < batch; b++)
		if (overlap(dst, dst_extent, (const char *)src + (size_t)b * batch_stride, src_frame))
			return fail("window: the destination overlaps source frame %d", b);
	// the regions of LL(l): LH(l) spans their columns, HL(l) their rows (a line has two samples or more at every level)
	c->x[c->r] = x0, c->nx[c->r] = w, c->y[c->r] = y0, c->ny[c->r] = h;
	for (int l = c->r + 1; l <= c->J; l++) {
		const int *hl = c->xywh + 4 * (3 * (l - 1) + 0), *lh = c->xywh + 4 * (3 * (l - 1) + 1);
		c->x[l] = lh[0], c->nx[l] = lh[2], c->y[l] = hl[1], c->ny[l] = hl[3];
		if (c->nx[l] <= 0 || c->ny[l] <= 0)
			return fail("window: empty region at level %d", l);
	}
	return 0;
}

// route 0: the full inverse of the top-left Wo(r) x Ho(r) rectangle at J - r levels into scratch, then the window's copy
int window_by_inverse(const WindowCall &c, const char *src, long bs, int batch, long sx, int size_x, int size_y, int x0, int y0, int w, int h,
	char *dst, long dbs, long dsx)
{
	const int es = c.es, Wr = ceil_div_pow2(size_x, c.r), Hr = ceil_div_pow2(size_y, c.r), levels = c.J - c.r;
	const long pitch = frame_pitch(es, Wr), frame = pitch * Hr;
	if (grow(g.win_ws, (size_t)frame * batch))
		return 1;
	char *ws = (char *)g.win_ws.p;
	const Geom ge{Wr, Hr, Wr, Hr};
	const Call2d c2 = call2d(c.w, {src, ws}, {sx, bs, pitch});
	bool batched = !c2.line_passes_only();
	for (int j = 0; j < levels; j++)
		batched = batched && level_fused_ok(c2, ge, j);
	if (batched || batch == 1) {
		if (inverse2d(c2, Img{(char *)src, sx, es}, Img{ws, pitch, es}, ge, levels, 0, 0, batch, bs, frame))
			return 1;
	} else {
		// (the exact line passes run image by image)
		for (int b = 0; b < batch; b++)
			if (inverse2d(c2, Img{(char *)src + b * bs, sx, es}, Img{ws + b * frame, pitch, es}, ge, levels, 0, 0, 1, 0, 0))
				return 1;
	}
	return launched(launch_window_copy(es, ws + y0 * pitch + (long)x0 * es, pitch / es, frame / es, dst, dsx / es, dbs / es, w, h, batch, g.stream),
		"window", "copy");
}

// route 2: one launch of the window kernel per level
int window_by_kernels(const WindowCall &c, const char *src, long bs, int batch, long sx, int size_x, int size_y, char *dst, long dbs, long dsx)
{
	const int es = c.es;
	// the regions between the levels: LL(J-1), LL(J-3), ... in the first half of the scratch, the others in the second
	size_t half = 0;
	for (int l = c.r + 1; l < c.J; l++)
		half = std::max(half, (size_t)frame_pitch(es, c.nx[l]) * c.ny[l] * batch);
	if (half && grow(g.win_ws, 2 * half))
		return 1;
	const char *ll = src;
	long ll_pitch = sx, ll_bs = bs;
	int ll_x0 = 0, ll_y0 = 0;
	for (int l = c.J; l > c.r; l--) {
		WindowLevelArgs a{};
		a.ll = ll, a.ll_pitch = ll_pitch / es, a.ll_bs = ll_bs / es, a.ll_x0 = ll_x0, a.ll_y0 = ll_y0;
		a.det = src, a.det_pitch = sx / es, a.det_bs = bs / es;
		a.W = ceil_div_pow2(size_x, l - 1), a.H = ceil_div_pow2(size_y, l - 1);
		a.Wd = ceil_div_pow2(size_x, l), a.Hd = ceil_div_pow2(size_y, l);
		a.xa = c.x[l - 1], a.xb = c.x[l - 1] + c.nx[l - 1], a.ya = c.y[l - 1], a.yb = c.y[l - 1] + c.ny[l - 1];
		a.batch = batch;
		if (l - 1 == c.r) {
			a.out = dst, a.out_pitch = dsx / es, a.out_bs = dbs / es;
		} else {
			const long pitch = frame_pitch(es, c.nx[l - 1]);
			char *buf = (char *)g.win_ws.p + ((c.J - l) & 1) * half;
			a.out = buf, a.out_pitch = pitch / es, a.out_bs = pitch * c.ny[l - 1] / es;
			ll = buf, ll_pitch = pitch, ll_bs = pitch * c.ny[l - 1], ll_x0 = a.xa, ll_y0 = a.ya;
		}
		if (launched(launch_window_level(c.w, a, g.stream), "window", "level"))
			return 1;
	}
	return 0;
}

} // namespace

} // namespace dwtb

using namespace dwtb;

#pragma GCC visibility push(default)
extern "C" {

int dwt_hip_inverse_window_batch(int wavelet, const void *src, size_t batch_stride, int batch, int stride_x, int size_x, int size_y, int j_max,
	int discard, int x0, int y0, int w, int h, void *dst, size_t dst_batch_stride, int dst_stride_x)
{
	static thread_local WindowCall c;
	if (window_check(&c, wavelet, src, batch_stride, batch, stride_x, size_x, size_y, j_max, discard, x0, y0, w, h, dst, dst_batch_stride,
			dst_stride_x))
		return 1;
	if (check_inited())
		return 1;
	if (!dwt_hip_is_device_pointer(src) || !dwt_hip_is_device_pointer(dst))
		return fail("window: the frames and the windows lie in device memory");
	const long bs = batch > 1 ? (long)batch_stride : 0, dbs = batch > 1 ? (long)dst_batch_stride : 0;
	if (c.J == c.r) // nothing to undo: the window of LL(J)
		return launched(launch_window_copy(c.es, (const char *)src + (long)y0 * stride_x + (long)x0 * c.es, stride_x / c.es, bs / c.es, dst,
					dst_stride_x / c.es, dbs / c.es, w, h, batch, g.stream),
			"window", "copy");
	const bool kernels = g.window_fused >= 2 || (g.window_fused == 1 && window_pays(c, size_x, size_y, w, h, batch));
	return kernels ? window_by_kernels(c, (const char *)src, bs, batch, stride_x, size_x, size_y, (char *)dst, dbs, dst_stride_x)
	               : window_by_inverse(c, (const char *)src, bs, batch, stride_x, size_x, size_y, x0, y0, w, h, (char *)dst, dbs, dst_stride_x);
}

int dwt_hip_window_route(int wavelet, int batch, int size_x, int size_y, int j_max, int discard, int x0, int y0, int w, int h)
{
	static thread_local WindowCall c;
	const int ns = dwt_hip_window_regions(wavelet, size_x, size_y, j_max, discard, x0, y0, w, h, c.xywh);
	if (ns < 0 || batch < 1)
		return -1;
	c.J = (ns - 1) / 3, c.r = discard;
	if (c.J == c.r)
		return 0;
	return g.window_fused >= 2 || (g.window_fused == 1 && window_pays(c, size_x, size_y, w, h, batch)) ? 2 : 0;
}

} // extern "C"
#pragma GCC visibility pop
