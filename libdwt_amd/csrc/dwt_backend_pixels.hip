// dwt_backend_pixels.hip -- the pixel front end: pictures of 8- / 16-bit unsigned pixels <-> wavelet planes, alone and
// composed with the batched 2-D transform, and their C-ABI (include/libdwt_hip.h).
//
// One call is one launch of k_pixels (dwt_pixels.hip) on the context's stream.  Each side of a call lies in host or in
// device memory.  A host side is mirrored: the bytes of its whole region cross PCIe once into a device buffer of the
// context, the kernel runs on the mirror, and a written side crosses back -- a written side whose region has bytes that
// are not the frame's own is uploaded first, so that those bytes return as they were.  A call with a host side ends
// synchronised; a call on device memory is ordered on the stream and waits for nothing.
//
// The composite entries go through a scratch stack of planes T with the caller's pitches (the batched transform does not
// run in place, and takes one row pitch and one batch stride for both sides): forward pixels -> T -> planes, inverse
// planes -> T -> pixels.  The caller's planes are only read by the inverse.
#include "dwt_backend.h"

#include <climits>

namespace dwtb {

namespace {

static_assert(PIXELS_PER_LANE == DWT_HIP_PIXELS_PER_LANE && PIXELS_GRID_ROWS == DWT_HIP_PIXELS_GRID_ROWS && PIXELS_GRID_BATCH == DWT_HIP_PIXELS_GRID_BATCH,
	"the header states the kernel's constants");
static_assert((int)kPlaneI16 == DWT_HIP_PLANE_I16 && (int)kPlaneI32 == DWT_HIP_PLANE_I32 && (int)kPlaneH == DWT_HIP_PLANE_H && (int)kPlaneS == DWT_HIP_PLANE_S,
	"plane types");

// a checked call: the kernel's arguments on the caller's pointers, and what the driver needs beyond them
struct PixCall {
	PixelsArgs a;
	int pt, plane, es;
	bool inverse;
	Side pix, planes;
};

// Which side moves by 16-byte accesses (dwt_pixels.hip) -- from addresses and strides alone.  Strides that the call does
// not use (one picture, one row, one channel, one plane) arrive as 0.
void pixels_route(PixelsArgs *a, int pt, bool inverse)
{
	const bool want = g.pixels_wide != 0;
	a->pix_al2 = ((uintptr_t)a->pix | a->pix_bs | a->pix_pitch | a->pix_stride | a->chan_stride) % 2 == 0;
	int layout = -1;
	if (a->pix_stride == pt)
		layout = 0; // a run of adjacent elements per channel: planar, grey
	else if ((a->channels == 1 || a->chan_stride == pt) && (a->pix_stride == 3 * pt || a->pix_stride == 4 * pt) && a->channels <= a->pix_stride / pt)
		layout = (int)(a->pix_stride / pt);
	a->layout = layout < 0 ? 0 : layout;
	a->wide_pix = want && layout >= 0 && all16({(uintptr_t)a->pix, (uintptr_t)a->pix_bs, (uintptr_t)a->pix_pitch}) &&
	              (layout != 0 || a->chan_stride % 16 == 0) &&
	              (!inverse || layout == 0 || a->channels == layout); // (an interleaved run is stored whole: every element a channel)
	a->wide_planes = want && all16({(uintptr_t)a->planes, (uintptr_t)a->plane_stride, (uintptr_t)a->plane_pitch});
}

int plane_of_wavelet(int wavelet, int *plane)
{
	switch (wavelet) {
	case DWT_HIP_CDF53_I16: *plane = DWT_HIP_PLANE_I16; return 0;
	case DWT_HIP_CDF53_I:
	case DWT_HIP_CDF97_I: *plane = DWT_HIP_PLANE_I32; return 0;
	case DWT_HIP_CDF97_H: *plane = DWT_HIP_PLANE_H; return 0;
	case DWT_HIP_CDF97_S:
	case DWT_HIP_CDF53_S:
	case DWT_HIP_INTERP53_S: *plane = DWT_HIP_PLANE_S; return 0;
	case DWT_HIP_CDF97_D:
	case DWT_HIP_CDF53_D: return fail("pictures: the double wavelets have no plane type (wavelet %d)", wavelet);
	}
	return fail("pictures: unknown wavelet %d", wavelet);
}

// every refusal of the header, before anything is written
int pixels_check(PixCall *c, bool inverse, int fmt, const void *pix, size_t pix_bs, size_t pix_pitch, size_t pix_stride, size_t chan_stride,
	int batch, int channels, int order, int depth, int offset, float scale, int colour, int plane, const void *planes, size_t plane_stride,
	size_t plane_pitch, int W, int H)
{
	if (fmt != DWT_HIP_PIX_U8 && fmt != DWT_HIP_PIX_U16)
		return fail("pixels: unknown pixel format %d", fmt);
	if (plane != DWT_HIP_PLANE_I16 && plane != DWT_HIP_PLANE_I32 && plane != DWT_HIP_PLANE_H && plane != DWT_HIP_PLANE_S)
		return fail("pixels: unknown plane type %d", plane);
	const int pt = fmt == DWT_HIP_PIX_U8 ? 1 : 2, es = plane == DWT_HIP_PLANE_I16 || plane == DWT_HIP_PLANE_H ? 2 : 4;
	const bool flt = plane == DWT_HIP_PLANE_H || plane == DWT_HIP_PLANE_S;
	if (channels != 1 && channels != 3 && channels != 4)
		return fail("pixels: %d channels (a picture has 1, 3 or 4)", channels);
	if (depth < 1 || depth > 8 * pt)
		return fail("pixels: depth %d (%d-bit pixels take 1 .. %d)", depth, 8 * pt, 8 * pt);
	if (order != DWT_HIP_ORDER_RGB && order != DWT_HIP_ORDER_BGR)
		return fail("pixels: unknown channel order %d", order);
	if (colour != DWT_HIP_COLOUR_NONE && colour != DWT_HIP_COLOUR_RCT && colour != DWT_HIP_COLOUR_ICT)
		return fail("pixels: unknown component transform %d", colour);
	if (colour == DWT_HIP_COLOUR_RCT && flt)
		return fail("pixels: the RCT takes integer planes (DWT_HIP_PLANE_I16, _I32)");
	if (colour == DWT_HIP_COLOUR_ICT && !flt)
		return fail("pixels: the ICT takes float planes (DWT_HIP_PLANE_H, _S)");
	if (!flt && scale != 1.0f)
		return fail("pixels: integer planes take scale 1 (got %g)", (double)scale);
	if (colour != DWT_HIP_COLOUR_NONE && channels < 3)
		return fail("pixels: a component transform takes 3 or 4 channels (got %d)", channels);
	if (colour == DWT_HIP_COLOUR_RCT && plane == DWT_HIP_PLANE_I16 && depth == 16)
		return fail("pixels: the RCT of 16-bit pixels needs 17 bits: take DWT_HIP_PLANE_I32");
	if (batch < 0 || W < 1 || H < 1)
		return fail("pixels: bad arguments (%d pictures of %d x %d)", batch, W, H);
	if (!pix || !planes)
		return fail("null pointer argument");
	const size_t lim = (size_t)1 << 46;
	if (pix_bs > lim || pix_pitch > lim || pix_stride > lim || chan_stride > lim || plane_stride > lim || plane_pitch > lim)
		return fail("pixels: bad strides");

	PixelsArgs &a = c->a;
	a = PixelsArgs{};
	a.pix = (char *)pix, a.planes = (char *)planes;
	a.batch = batch, a.channels = channels, a.W = W, a.H = H;
	// a stride that no element is reached by does not count
	a.pix_bs = batch > 1 ? (long)pix_bs : 0, a.pix_pitch = H > 1 ? (long)pix_pitch : 0;
	a.pix_stride = W > 1 ? (long)pix_stride : pt, a.chan_stride = channels > 1 ? (long)chan_stride : 0;
	const long n_planes = (long)batch * channels;
	a.plane_stride = n_planes > 1 ? (long)plane_stride : 0, a.plane_pitch = H > 1 ? (long)plane_pitch : 0;
	a.bgr = order == DWT_HIP_ORDER_BGR, a.colour = colour != DWT_HIP_COLOUR_NONE;
	a.offset = offset, a.maxv = (1 << depth) - 1, a.scale = scale;

	// no two elements of a picture share a byte: the three steps (pixel, channel, row), smallest first, are nested
	struct Dim {
		long count, stride;
	} d[3] = {{W, a.pix_stride}, {channels, a.chan_stride}, {H, a.pix_pitch}};
	std::sort(d, d + 3, [](const Dim &x, const Dim &y) { return (x.count > 1 ? x.stride : 0) < (y.count > 1 ? y.stride : 0); });
	long pic = pt;
	for (const Dim &k : d) {
		if (k.count < 2)
			continue;
		if (k.stride < pic)
			return fail("pixels: the elements of a picture overlap (pixel step %zu, channel step %zu, row pitch %zu bytes)", pix_stride,
				chan_stride, pix_pitch);
		if (!mul_add(&pic, k.count - 1, k.stride))
			return fail("pixels: bad strides");
	}
	if (batch > 1 && a.pix_bs < pic)
		return fail("pixels: pictures must be apart (batch stride %zu bytes, a picture takes %ld)", pix_bs, pic);
	long pix_extent = pic;
	if (!mul_add(&pix_extent, std::max(batch - 1, 0), a.pix_bs))
		return fail("pixels: bad strides");

	if ((uintptr_t)planes % es || a.plane_stride % es || a.plane_pitch % es)
		return fail("pixels: plane addresses and strides are multiples of the element size (%d bytes)", es);
	const long row = (long)W * es;
	long one = row;
	if ((H > 1 && a.plane_pitch < row) || !mul_add(&one, H - 1, a.plane_pitch))
		return fail("pixels: bad plane row pitch (%zu bytes for %d elements of %d)", plane_pitch, W, es);
	if (n_planes > 1 && a.plane_stride < one)
		return fail("pixels: planes must be apart (plane stride %zu bytes, a plane takes %ld)", plane_stride, one);
	long plane_extent = one;
	if (!mul_add(&plane_extent, std::max(n_planes - 1, 0l), a.plane_stride))
		return fail("pixels: bad strides");
	if (batch > 0 && overlap(pix, (size_t)pix_extent, planes, (size_t)plane_extent))
		return fail("pixels: the pixels and the planes must not overlap");

	c->pt = pt, c->plane = plane, c->es = es, c->inverse = inverse;
	// dense: the region holds nothing but the frame (the nested steps close up)
	long fill = pt;
	bool dense = true;
	for (const Dim &k : d)
		if (k.count > 1)
			dense = dense && k.stride == fill, fill *= k.count;
	dense = dense && (batch < 2 || a.pix_bs == pic);
	c->pix = Side{pix, (size_t)pix_extent, dense};
	c->planes = Side{planes, (size_t)plane_extent, (H < 2 || a.plane_pitch == row) && (n_planes < 2 || a.plane_stride == one)};
	return 0;
}

int convert(const PixCall &c, char *pix, char *planes)
{
	PixelsArgs a = c.a;
	a.pix = pix, a.planes = planes;
	pixels_route(&a, c.pt, c.inverse);
	a.nt_out = nt_for(c.inverse ? c.pix.extent : c.planes.extent);
	return launched(launch_pixels(c.pt, c.plane, c.inverse, a, g.stream), "pixels", c.inverse ? "planes to pixels" : "pixels to planes");
}

// wavelet < 0: the conversion alone
int pixels_call(PixCall &c, int wavelet, int *j)
{
	if (c.a.batch == 0)
		return 0;
	bool composite = wavelet >= 0;
	const long n_planes = (long)c.a.batch * c.a.channels;
	if (composite) {
		if (n_planes > 65535)
			return fail("pictures: %d pictures of %d channels are %ld planes (the batched transform takes 65535)", c.a.batch, c.a.channels, n_planes);
		if (!j)
			return fail("null pointer argument");
		// (what dwt_hip_transform2d_batch asks of its strides, asked here before anything is written)
		if (c.a.plane_pitch == 0)
			c.a.plane_pitch = (long)c.a.W * c.es;
		if (c.a.plane_pitch > INT_MAX)
			return fail("pictures: the batched transform takes a row pitch below 2 GiB (got %ld bytes)", c.a.plane_pitch);
		if (c.a.plane_stride < c.a.plane_pitch * c.a.H) {
			if (n_planes > 1)
				return fail("pictures: planes must be whole rows apart (plane stride %ld bytes, %d rows of %ld)", c.a.plane_stride, c.a.H,
					c.a.plane_pitch);
			c.a.plane_stride = c.a.plane_pitch * c.a.H;
		}
		// The levels the transform will run, by its own clamp (forward2d / inverse2d).  None -- *j == 0, or a picture one
		// pixel wide or high -- and the transform is the identity, which its drivers do not copy for a batch: the call is the
		// conversion between the pixels and the caller's planes, without the scratch stack.
		const int lim = ceil_log2(std::min(c.a.W, c.a.H));
		const int levels = c.inverse ? (*j >= 0 && *j < lim ? *j : lim) : (*j < 0 || *j > lim ? lim : *j);
		if (levels == 0) {
			composite = false;
			if (!c.inverse)
				*j = 0;
		}
	}
	if (check_inited())
		return 1;
	char *pix, *planes;
	bool pix_host, planes_host;
	if (mirror(c.pix, g.px_pix, !c.inverse || !c.pix.dense, &pix, &pix_host) ||
	    mirror(c.planes, g.px_planes, c.inverse || !c.planes.dense, &planes, &planes_host))
		return 1;
	if (!composite) {
		if (convert(c, pix, planes))
			return 1;
	} else {
		if (grow(g.px_tmp, (size_t)n_planes * c.a.plane_stride))
			return 1;
		char *const T = (char *)g.px_tmp.p;
		if (!c.inverse) {
			if (convert(c, pix, T) ||
			    dwt_hip_transform2d_batch(wavelet, 0, T, planes, (size_t)c.a.plane_stride, (int)n_planes, (int)c.a.plane_pitch, c.a.W, c.a.H, j))
				return 1;
		} else {
			if (dwt_hip_transform2d_batch(wavelet, 1, planes, T, (size_t)c.a.plane_stride, (int)n_planes, (int)c.a.plane_pitch, c.a.W, c.a.H, j) ||
			    convert(c, pix, T))
				return 1;
		}
	}
	if (c.inverse ? pix_host : planes_host) {
		if (c.inverse ? mirror_back(c.pix, g.px_pix) : mirror_back(c.planes, g.px_planes))
			return 1;
	}
	if (pix_host || planes_host)
		HIP_TRY(hipStreamSynchronize(g.stream));
	return 0;
}

} // namespace

// a host side's mirror in `buf`; *dev: where the kernel finds the side
int mirror(const Side &s, Buf &buf, bool upload, char **dev, bool *is_host)
{
	*is_host = !dwt_hip_is_device_pointer(s.p);
	*dev = (char *)s.p;
	if (!*is_host)
		return 0;
	if (grow(buf, s.extent))
		return 1;
	*dev = (char *)buf.p;
	if (upload)
		HIP_TRY(hipMemcpyAsync(buf.p, s.p, s.extent, hipMemcpyHostToDevice, g.stream));
	return 0;
}

int mirror_back(const Side &s, const Buf &buf)
{
	HIP_TRY(hipMemcpyAsync((void *)s.p, buf.p, s.extent, hipMemcpyDeviceToHost, g.stream));
	return 0;
}

} // namespace dwtb

using namespace dwtb;

#pragma GCC visibility push(default)
extern "C" {

int dwt_hip_pixels_to_planes_batch(int fmt, const void *pix, size_t pix_batch_stride, size_t pix_row_pitch, size_t pix_stride,
	size_t chan_stride, int batch, int channels, int order, int depth, int offset, float scale, int colour, int plane_type, void *planes,
	size_t plane_stride, size_t plane_row_pitch, int size_x, int size_y)
{
	PixCall c;
	if (pixels_check(&c, false, fmt, pix, pix_batch_stride, pix_row_pitch, pix_stride, chan_stride, batch, channels, order, depth, offset, scale,
			colour, plane_type, planes, plane_stride, plane_row_pitch, size_x, size_y))
		return 1;
	return pixels_call(c, -1, nullptr);
}

int dwt_hip_planes_to_pixels_batch(int fmt, void *pix, size_t pix_batch_stride, size_t pix_row_pitch, size_t pix_stride, size_t chan_stride,
	int batch, int channels, int order, int depth, int offset, float scale, int colour, int plane_type, const void *planes, size_t plane_stride,
	size_t plane_row_pitch, int size_x, int size_y)
{
	PixCall c;
	if (pixels_check(&c, true, fmt, pix, pix_batch_stride, pix_row_pitch, pix_stride, chan_stride, batch, channels, order, depth, offset, scale,
			colour, plane_type, planes, plane_stride, plane_row_pitch, size_x, size_y))
		return 1;
	return pixels_call(c, -1, nullptr);
}

int dwt_hip_picture_forward_batch(int wavelet, int fmt, const void *pix, size_t pix_batch_stride, size_t pix_row_pitch, size_t pix_stride,
	size_t chan_stride, int batch, int channels, int order, int depth, int offset, float scale, int colour, void *planes, size_t plane_stride,
	size_t plane_row_pitch, int size_x, int size_y, int *j)
{
	PixCall c;
	int plane;
	if (plane_of_wavelet(wavelet, &plane) ||
	    pixels_check(&c, false, fmt, pix, pix_batch_stride, pix_row_pitch, pix_stride, chan_stride, batch, channels, order, depth, offset, scale,
			colour, plane, planes, plane_stride, plane_row_pitch, size_x, size_y))
		return 1;
	return pixels_call(c, wavelet, j);
}

int dwt_hip_picture_inverse_batch(int wavelet, int fmt, void *pix, size_t pix_batch_stride, size_t pix_row_pitch, size_t pix_stride,
	size_t chan_stride, int batch, int channels, int order, int depth, int offset, float scale, int colour, const void *planes,
	size_t plane_stride, size_t plane_row_pitch, int size_x, int size_y, int j)
{
	PixCall c;
	int plane;
	if (plane_of_wavelet(wavelet, &plane) ||
	    pixels_check(&c, true, fmt, pix, pix_batch_stride, pix_row_pitch, pix_stride, chan_stride, batch, channels, order, depth, offset, scale,
			colour, plane, planes, plane_stride, plane_row_pitch, size_x, size_y))
		return 1;
	return pixels_call(c, wavelet, &j);
}

int dwt_hip_pixels_route(int fmt, int inverse, const void *pix, size_t pix_batch_stride, size_t pix_row_pitch, size_t pix_stride,
	size_t chan_stride, int batch, int channels, int plane_type, const void *planes, size_t plane_stride, size_t plane_row_pitch, int size_x,
	int size_y)
{
	PixCall c;
	if (pixels_check(&c, inverse != 0, fmt, pix, pix_batch_stride, pix_row_pitch, pix_stride, chan_stride, batch, channels, DWT_HIP_ORDER_RGB,
			1, 0, 1.0f, DWT_HIP_COLOUR_NONE, plane_type, planes, plane_stride, plane_row_pitch, size_x, size_y))
		return -1;
	pixels_route(&c.a, c.pt, c.inverse);
	return (c.a.wide_pix ? DWT_HIP_PIXELS_WIDE_PIX : 0) | (c.a.wide_planes ? DWT_HIP_PIXELS_WIDE_PLANES : 0);
}

} // extern "C"
#pragma GCC visibility pop
