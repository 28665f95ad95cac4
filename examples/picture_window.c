/*
 * picture_window.c -- viewports of a colour picture that stays on the device as wavelet planes
 * (dwt_hip_inverse_window_batch, an extension of this library).  A synthetic RGB8 picture goes through the
 * pixel front end once (level shift, RCT, int16 CDF 5/3: dwt_hip_picture_forward_batch).  Then, without the full inverse
 * and without a destination as large as the picture,
 *   1. a viewport at full resolution (discard 0) and
 *   2. a viewport of the picture at a quarter of its resolution (discard 2: LL(2), the two finest levels never read)
 * are decoded: the windowed inverse of the three planes into three small planes, and dwt_hip_planes_to_pixels_batch on
 * those.  Each must be pixel for pixel the crop of the full picture inverse -- of the picture's top-left LL(2)-sized
 * rectangle at two levels fewer for the second.  Prints the bytes of coefficients the viewports depend on
 * (dwt_hip_window_regions) against the frame's.  Own code written against include/libdwt_hip.h.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/picture_window.c -o picture_window \
 *       -Llibdwt_amd -l:libdwt_hip.so -Wl,-rpath,$PWD/libdwt_amd -lm
 *   ./picture_window
 */
#include "libdwt.h"
#include "libdwt_hip.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static unsigned char *synthetic(int w, int h)
{
	unsigned char *pix = malloc((size_t)w * h * 3);
	unsigned s = 12345u;
	for (int y = 0; pix && y < h; y++)
		for (int x = 0; x < w; x++) {
			unsigned char *p = pix + 3 * ((size_t)y * w + x);
			s = s * 1664525u + 1013904223u; /* a gradient, a pattern and some noise: all 256 values occur */
			p[0] = (unsigned char)(255 * x / (w - 1));
			p[1] = (unsigned char)((x ^ y) & 255);
			p[2] = (unsigned char)(((255 * y / (h - 1)) + (s >> 28)) & 255);
		}
	return pix;
}

/* One viewport [x0, x0 + vw) x [y0, y0 + vh) of LL(discard) as pixels: the windowed inverse of the three planes, then the
 * conversion of the small planes.  Returns the pixels that differ from the crop of `full` (rows of full_w pixels). */
static long viewport(const void *d_planes, size_t plane, size_t plane_pitch, int w, int h, int j, int discard, int x0, int y0, int vw, int vh,
	const unsigned char *full, int full_w, long *region_bytes)
{
	const size_t small_pitch = (size_t)vw * 2, small = small_pitch * vh, n = (size_t)vw * vh * 3;
	void *d_small = dwt_hip_malloc(3 * small), *d_view = dwt_hip_malloc(n);
	unsigned char *view = malloc(n);
	if (!d_small || !d_view || !view)
		dwt_util_error("allocation failed: %s\n", dwt_hip_last_error());
	/* the three planes are a batch of three frames, plane bytes apart */
	if (dwt_hip_inverse_window_batch(DWT_HIP_CDF53_I16, d_planes, plane, 3, (int)plane_pitch, w, h, j, discard, x0, y0, vw, vh, d_small, small,
			(int)small_pitch) ||
	    dwt_hip_planes_to_pixels_batch(DWT_HIP_PIX_U8, d_view, n, (size_t)vw * 3, 3, 1, 1, 3, DWT_HIP_ORDER_RGB, 8, 128, 1.0f, DWT_HIP_COLOUR_RCT,
			DWT_HIP_PLANE_I16, d_small, small, small_pitch, vw, vh))
		dwt_util_error("viewport: %s\n", dwt_hip_last_error());
	dwt_hip_memcpy_d2h(view, d_view, n);
	long differ = 0;
	for (int y = 0; y < vh; y++)
		for (int x = 0; x < vw; x++)
			differ += memcmp(view + 3 * ((size_t)y * vw + x), full + 3 * ((size_t)(y0 + y) * full_w + x0 + x), 3) != 0;
	int xywh[4 * DWT_HIP_BAND_MAX_SLOTS];
	const int slots = dwt_hip_window_regions(DWT_HIP_CDF53_I16, w, h, j, discard, x0, y0, vw, vh, xywh);
	*region_bytes = 0;
	for (int k = 0; k < slots; k++)
		*region_bytes += 3l * 2 * xywh[4 * k + 2] * xywh[4 * k + 3];
	dwt_hip_free(d_small);
	dwt_hip_free(d_view);
	free(view);
	return differ;
}

int main(void)
{
	dwt_util_init();
	dwt_util_log(LOG_INFO, "library: %s on %s\n", dwt_util_version(), dwt_hip_device_name());

	const int w = 1000, h = 700;
	unsigned char *pix = synthetic(w, h);
	const size_t n = (size_t)w * h * 3, row = (size_t)w * 3, plane_pitch = (size_t)w * 2, plane = plane_pitch * h;
	unsigned char *full = malloc(n);
	void *d_pix = dwt_hip_malloc(n), *d_full = dwt_hip_malloc(n), *d_planes = dwt_hip_malloc(3 * plane);
	if (!pix || !full || !d_pix || !d_full || !d_planes)
		dwt_util_error("allocation failed: %s\n", dwt_hip_last_error());
	dwt_hip_memcpy_h2d(d_pix, pix, n);
	int j = 5;
	if (dwt_hip_picture_forward_batch(DWT_HIP_CDF53_I16, DWT_HIP_PIX_U8, d_pix, n, row, 3, 1, 1, 3, DWT_HIP_ORDER_RGB, 8, 128, 1.0f,
			DWT_HIP_COLOUR_RCT, d_planes, plane, plane_pitch, w, h, &j))
		dwt_util_error("forward: %s\n", dwt_hip_last_error());
	const long frame_bytes = 3l * (long)plane;
	long region_bytes, bad = 0;

	/* 1. full resolution: the crop of the full picture inverse */
	if (dwt_hip_picture_inverse_batch(DWT_HIP_CDF53_I16, DWT_HIP_PIX_U8, d_full, n, row, 3, 1, 1, 3, DWT_HIP_ORDER_RGB, 8, 128, 1.0f,
			DWT_HIP_COLOUR_RCT, d_planes, plane, plane_pitch, w, h, j))
		dwt_util_error("inverse: %s\n", dwt_hip_last_error());
	dwt_hip_memcpy_d2h(full, d_full, n);
	if (memcmp(full, pix, n))
		dwt_util_error("the full inverse does not give the picture back\n");
	long differ = viewport(d_planes, plane, plane_pitch, w, h, j, 0, 401, 233, 256, 192, full, w, &region_bytes);
	printf("viewport 256 x 192 at (401, 233) of %d x %d, discard 0: %ld pixels differ; regions %ld bytes of %ld (%.1f %%)\n", w, h, differ,
		region_bytes, frame_bytes, 100.0 * region_bytes / frame_bytes);
	bad += differ;

	/* 2. a quarter of the resolution: LL(2) is the picture of 250 x 175; its full inverse runs on the top-left rectangle */
	const int w2 = (w + 3) / 4, h2 = (h + 3) / 4;
	if (dwt_hip_picture_inverse_batch(DWT_HIP_CDF53_I16, DWT_HIP_PIX_U8, d_full, (size_t)w2 * h2 * 3, (size_t)w2 * 3, 3, 1, 1, 3,
			DWT_HIP_ORDER_RGB, 8, 128, 1.0f, DWT_HIP_COLOUR_RCT, d_planes, plane, plane_pitch, w2, h2, j - 2))
		dwt_util_error("inverse at a quarter of the resolution: %s\n", dwt_hip_last_error());
	dwt_hip_memcpy_d2h(full, d_full, (size_t)w2 * h2 * 3);
	differ = viewport(d_planes, plane, plane_pitch, w, h, j, 2, 97, 40, 128, 96, full, w2, &region_bytes);
	printf("viewport 128 x 96 at (97, 40) of LL(2), %d x %d, discard 2: %ld pixels differ; regions %ld bytes of %ld (%.1f %%)\n", w2, h2, differ,
		region_bytes, frame_bytes, 100.0 * region_bytes / frame_bytes);
	bad += differ;

	dwt_hip_free(d_pix);
	dwt_hip_free(d_full);
	dwt_hip_free(d_planes);
	free(pix);
	free(full);
	dwt_util_finish();
	printf("%s\n", bad ? "viewports DIFFER" : "viewports identical");
	return bad ? 1 : 0;
}
