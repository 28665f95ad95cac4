// dwt_pixels.hip -- the pixel front end ON THE DEVICE: 8- / 16-bit unsigned pixels <-> wavelet planes (int16, int32,
// binary16, binary32) with the DC level shift and the component transforms of ITU-T T.800 Annex G (RCT, ICT).
// include/libdwt_hip.h states the arithmetic; DESIGN.md s25 the kernel.
//
// A lane converts PIXELS_PER_LANE = 16 consecutive pixels of one row, a wave 1024 pixels of one row, a workgroup of four
// waves four rows.  Each side of a lane's run moves by one of two routes, chosen per side on the host (pixels_route):
//   wide:    16-byte accesses.  A run of 16 pixels is 16 * pix_stride bytes (interleaved: RGB8 three loads, BGRA8 four) or
//            16 elements per channel (planar); 16 plane elements are two (int16, binary16) or four (int32, binary32)
//            16-byte stores.  Takes 16-byte aligned bases, pitches and strides; the lane's run then starts on a 16-byte
//            boundary because its first pixel is a multiple of 16.
//            A forward load of an interleaved pixel with more elements than channels (three channels of a 4-element
//            pixel, grey at a 3- or 4-element step) brings the unused elements along: for the last pixel of a frame up to
//            3 (u8) or 6 (u16) bytes past the frame's last element, inside the same aligned 16 bytes.  Read, never used,
//            never written.
//   element: one access per element (per byte for 16-bit pixels on odd addresses).  Everything else, and the last lane of a
//            row whose run is shorter than 16 pixels.
// Both routes fill the same registers, the arithmetic between them is one piece of code: same bits.
//
// Every product and sum of the ICT is rounded to binary32 on its own (no contraction: the Makefile's -ffp-contract=off,
// repeated below).  Bound by bytes: a lane holds 64 samples in registers, no LDS, no barrier.
#include "dwt_device.h"
#include "dwt_runs.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace dwt {

namespace {

constexpr int PPL = PIXELS_PER_LANE;

constexpr int plane_es(int plane) { return plane == kPlaneI16 || plane == kPlaneH ? 2 : 4; }

// one element on the element route.  Pixels: any byte address (16-bit ones by bytes unless al2); planes: element aligned
template <int PT>
static __device__ __forceinline__ unsigned pix_load(const char *p, bool al2)
{
	const unsigned char *b = (const unsigned char *)p;
	if constexpr (PT == 1)
		return b[0];
	else
		return al2 ? (unsigned)*(const unsigned short *)p : (unsigned)b[0] | (unsigned)b[1] << 8;
}
template <int PT>
static __device__ __forceinline__ void pix_store(char *p, unsigned v, bool al2)
{
	unsigned char *b = (unsigned char *)p;
	if constexpr (PT == 1) {
		b[0] = (unsigned char)v;
	} else {
		if (al2)
			*(unsigned short *)p = (unsigned short)v;
		else
			b[0] = (unsigned char)v, b[1] = (unsigned char)(v >> 8);
	}
}
template <int ES>
static __device__ __forceinline__ unsigned plane_load(const char *p)
{
	if constexpr (ES == 2)
		return *(const unsigned short *)p;
	else
		return *(const unsigned *)p;
}
template <int ES>
static __device__ __forceinline__ void plane_store(char *p, unsigned v)
{
	if constexpr (ES == 2)
		*(unsigned short *)p = (unsigned short)v;
	else
		*(unsigned *)p = v;
}

// the bits of a plane element <-> the sample
template <int PLANE>
static __device__ __forceinline__ int plane_int(unsigned bits)
{
	return PLANE == kPlaneI16 ? (int)(short)bits : (int)bits;
}
template <int PLANE>
static __device__ __forceinline__ float plane_float(unsigned bits)
{
	return PLANE == kPlaneH ? widen_h(bits) : from_bits<float>(bits);
}

static __device__ __forceinline__ int wrap_add(int a, int b) { return (int)((unsigned)a + (unsigned)b); }
static __device__ __forceinline__ int wrap_sub(int a, int b) { return (int)((unsigned)a - (unsigned)b); }

// a reconstructed float sample as a pixel: nearest integer (ties to even), + offset, clamped; NaN gives 0
static __device__ __forceinline__ unsigned float_pixel(float x, int offset, int maxv)
{
	const float r = __builtin_rintf(x);
	if (r != r)
		return 0;
	double t = (double)r + (double)offset; // (exact: r is an integer or past every pixel range)
	t = t < 0.0 ? 0.0 : t;
	t = t > (double)maxv ? (double)maxv : t;
	return (unsigned)(int)t;
}

template <int PT, int PLANE, bool INV>
__global__ __launch_bounds__(256) void k_pixels(PixelsArgs a)
{
	constexpr int ES = plane_es(PLANE);
	constexpr bool FLT = PLANE == kPlaneH || PLANE == kPlaneS;
	const int wave = threadIdx.x >> 6;
	const long x0 = ((long)blockIdx.x * 64 + (threadIdx.x & 63)) * PPL;
	if (x0 >= a.W)
		return;
	const int n = (int)min((long)PPL, a.W - x0);
	const bool wide_pix = a.wide_pix && n == PPL, wide_planes = a.wide_planes && n == PPL;
	const int ch = a.channels;

	for (int b = blockIdx.z; b < a.batch; b += gridDim.z)
		for (int y = blockIdx.y * PIXELS_WG_ROWS + wave; y < a.H; y += gridDim.y * PIXELS_WG_ROWS) {
			char *const px = a.pix + (long)b * a.pix_bs + (long)y * a.pix_pitch + x0 * a.pix_stride;
			char *const pl = a.planes + (long)b * ch * a.plane_stride + (long)y * a.plane_pitch + x0 * ES;
			unsigned pv[4][PPL]; // pixel values, channel order of the pixel
			unsigned pb[4][PPL]; // plane element bits, component order
#pragma unroll
			for (int c = 0; c < 4; c++)
#pragma unroll
				for (int i = 0; i < PPL; i++)
					pv[c][i] = pb[c][i] = 0;

			// ---- load
			if constexpr (!INV) {
				if (wide_pix) {
					if (a.layout == 3) {
						unsigned e[PPL * 3];
						run_load<PT>(px, e);
#pragma unroll
						for (int i = 0; i < PPL; i++)
							pv[0][i] = e[3 * i], pv[1][i] = e[3 * i + 1], pv[2][i] = e[3 * i + 2];
					} else if (a.layout == 4) {
						unsigned e[PPL * 4];
						run_load<PT>(px, e);
#pragma unroll
						for (int i = 0; i < PPL; i++)
							pv[0][i] = e[4 * i], pv[1][i] = e[4 * i + 1], pv[2][i] = e[4 * i + 2], pv[3][i] = e[4 * i + 3];
					} else {
#pragma unroll
						for (int c = 0; c < 4; c++)
							if (c < ch)
								run_load<PT>(px + c * a.chan_stride, pv[c]);
					}
				} else {
#pragma unroll
					for (int i = 0; i < PPL; i++)
#pragma unroll
						for (int c = 0; c < 4; c++)
							if (i < n && c < ch)
								pv[c][i] = pix_load<PT>(px + i * a.pix_stride + c * a.chan_stride, a.pix_al2);
				}
			} else {
				if (wide_planes) {
#pragma unroll
					for (int c = 0; c < 4; c++)
						if (c < ch)
							run_load<ES>(pl + c * a.plane_stride, pb[c]);
				} else {
#pragma unroll
					for (int c = 0; c < 4; c++)
#pragma unroll
						for (int i = 0; i < PPL; i++)
							if (i < n && c < ch)
								pb[c][i] = plane_load<ES>(pl + c * a.plane_stride + (long)i * ES);
				}
			}

			// ---- arithmetic (include/libdwt_hip.h): a pixel's channels 0 / 2 are R / B (order BGR: B / R)
#pragma unroll
			for (int i = 0; i < PPL; i++) {
				if constexpr (!INV) {
					const int v0 = wrap_sub((int)pv[0][i], a.offset), v1 = wrap_sub((int)pv[1][i], a.offset),
					          v2 = wrap_sub((int)pv[2][i], a.offset), v3 = wrap_sub((int)pv[3][i], a.offset);
					if constexpr (!FLT) {
						int o0 = v0, o1 = v1, o2 = v2;
						if (a.colour) { // RCT
							const int R = a.bgr ? v2 : v0, G = v1, B = a.bgr ? v0 : v2;
							o0 = wrap_add(wrap_add(R, wrap_add(G, G)), B) >> 2;
							o1 = wrap_sub(B, G);
							o2 = wrap_sub(R, G);
						}
						pb[0][i] = (unsigned)o0, pb[1][i] = (unsigned)o1, pb[2][i] = (unsigned)o2, pb[3][i] = (unsigned)v3;
					} else {
						const float f0 = (float)v0 * a.scale, f1 = (float)v1 * a.scale, f2 = (float)v2 * a.scale, f3 = (float)v3 * a.scale;
						float o0 = f0, o1 = f1, o2 = f2;
						if (a.colour) { // ICT
							const float R = a.bgr ? f2 : f0, G = f1, B = a.bgr ? f0 : f2;
							o0 = (0.299f * R + 0.587f * G) + 0.114f * B;
							o1 = (-0.16875f * R + -0.33126f * G) + 0.5f * B;
							o2 = (0.5f * R + -0.41869f * G) + -0.08131f * B;
						}
						if constexpr (PLANE == kPlaneH)
							pb[0][i] = narrow_h(o0), pb[1][i] = narrow_h(o1), pb[2][i] = narrow_h(o2), pb[3][i] = narrow_h(f3);
						else
							pb[0][i] = to_bits(o0), pb[1][i] = to_bits(o1), pb[2][i] = to_bits(o2), pb[3][i] = to_bits(f3);
					}
				} else {
					if constexpr (!FLT) {
						const int s0 = plane_int<PLANE>(pb[0][i]), s1 = plane_int<PLANE>(pb[1][i]), s2 = plane_int<PLANE>(pb[2][i]),
						          s3 = plane_int<PLANE>(pb[3][i]);
						int c0 = s0, c1 = s1, c2 = s2;
						if (a.colour) { // RCT: Y, U, V
							const int G = wrap_sub(s0, wrap_add(s1, s2) >> 2), R = wrap_add(s2, G), B = wrap_add(s1, G);
							c0 = a.bgr ? B : R, c1 = G, c2 = a.bgr ? R : B;
						}
						pv[0][i] = (unsigned)min(max(wrap_add(c0, a.offset), 0), a.maxv);
						pv[1][i] = (unsigned)min(max(wrap_add(c1, a.offset), 0), a.maxv);
						pv[2][i] = (unsigned)min(max(wrap_add(c2, a.offset), 0), a.maxv);
						pv[3][i] = (unsigned)min(max(wrap_add(s3, a.offset), 0), a.maxv);
					} else {
						const float s0 = plane_float<PLANE>(pb[0][i]), s1 = plane_float<PLANE>(pb[1][i]), s2 = plane_float<PLANE>(pb[2][i]),
						            s3 = plane_float<PLANE>(pb[3][i]);
						float c0 = s0, c1 = s1, c2 = s2;
						if (a.colour) { // ICT: Y, Cb, Cr
							const float R = s0 + 1.402f * s2;
							const float G = (s0 + -0.34413f * s1) + -0.71414f * s2;
							const float B = s0 + 1.772f * s1;
							c0 = a.bgr ? B : R, c1 = G, c2 = a.bgr ? R : B;
						}
						pv[0][i] = float_pixel(c0 * a.scale, a.offset, a.maxv);
						pv[1][i] = float_pixel(c1 * a.scale, a.offset, a.maxv);
						pv[2][i] = float_pixel(c2 * a.scale, a.offset, a.maxv);
						pv[3][i] = float_pixel(s3 * a.scale, a.offset, a.maxv);
					}
				}
			}

			// ---- store: the frame's own elements only
			if constexpr (!INV) {
				if (wide_planes) {
#pragma unroll
					for (int c = 0; c < 4; c++)
						if (c < ch)
							run_store<ES>(pl + c * a.plane_stride, pb[c], a.nt_out != 0);
				} else {
#pragma unroll
					for (int c = 0; c < 4; c++)
#pragma unroll
						for (int i = 0; i < PPL; i++)
							if (i < n && c < ch)
								plane_store<ES>(pl + c * a.plane_stride + (long)i * ES, pb[c][i]);
				}
			} else {
				if (wide_pix) { // (the host grants it to interleaved pixels only where every element of the pixel is a channel)
					if (a.layout == 3) {
						unsigned e[PPL * 3];
#pragma unroll
						for (int i = 0; i < PPL; i++)
							e[3 * i] = pv[0][i], e[3 * i + 1] = pv[1][i], e[3 * i + 2] = pv[2][i];
						run_store<PT>(px, e, a.nt_out != 0);
					} else if (a.layout == 4) {
						unsigned e[PPL * 4];
#pragma unroll
						for (int i = 0; i < PPL; i++)
							e[4 * i] = pv[0][i], e[4 * i + 1] = pv[1][i], e[4 * i + 2] = pv[2][i], e[4 * i + 3] = pv[3][i];
						run_store<PT>(px, e, a.nt_out != 0);
					} else {
#pragma unroll
						for (int c = 0; c < 4; c++)
							if (c < ch)
								run_store<PT>(px + c * a.chan_stride, pv[c], a.nt_out != 0);
					}
				} else {
#pragma unroll
					for (int i = 0; i < PPL; i++)
#pragma unroll
						for (int c = 0; c < 4; c++)
							if (i < n && c < ch)
								pix_store<PT>(px + i * a.pix_stride + c * a.chan_stride, pv[c][i], a.pix_al2);
				}
			}
		}
}

template <int PT, int PLANE>
hipError_t pixels_go(bool inverse, const PixelsArgs &a, dim3 grid, hipStream_t s)
{
	if (inverse)
		k_pixels<PT, PLANE, true><<<grid, 256, 0, s>>>(a);
	else
		k_pixels<PT, PLANE, false><<<grid, 256, 0, s>>>(a);
	return hipGetLastError();
}

template <int PT>
hipError_t pixels_go_plane(int plane, bool inverse, const PixelsArgs &a, dim3 grid, hipStream_t s)
{
	switch (plane) {
	case kPlaneI16: return pixels_go<PT, kPlaneI16>(inverse, a, grid, s);
	case kPlaneI32: return pixels_go<PT, kPlaneI32>(inverse, a, grid, s);
	case kPlaneH: return pixels_go<PT, kPlaneH>(inverse, a, grid, s);
	case kPlaneS: return pixels_go<PT, kPlaneS>(inverse, a, grid, s);
	}
	return hipErrorInvalidValue;
}

} // namespace

hipError_t launch_pixels(int pix_bytes, int plane, bool inverse, const PixelsArgs &a, hipStream_t s)
{
	if (a.W < 1 || a.H < 1 || a.batch < 1 || (a.channels != 1 && a.channels != 3 && a.channels != 4) || (pix_bytes != 1 && pix_bytes != 2))
		return hipErrorInvalidValue;
	// rows and pictures past the caps are taken by the kernel's own loops (tests/test_hip_pixels.py)
	const long gx = (a.W + 64l * PPL - 1) / (64l * PPL), gy = (a.H + PIXELS_WG_ROWS - 1) / PIXELS_WG_ROWS;
	const dim3 grid((unsigned)gx, (unsigned)std::min<long>(gy, PIXELS_GRID_ROWS / PIXELS_WG_ROWS), (unsigned)std::min(a.batch, PIXELS_GRID_BATCH));
	return pix_bytes == 1 ? pixels_go_plane<1>(plane, inverse, a, grid, s) : pixels_go_plane<2>(plane, inverse, a, grid, s);
}

} // namespace dwt
