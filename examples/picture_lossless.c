/*
 * picture_lossless.c -- a colour picture through the pixel front end (dwt_hip_picture_forward_batch / _inverse_batch, an
 * extension of this library).  Fills a synthetic RGB8 picture, or reads a binary PPM (P6, maxval 255),
 * uploads the bytes once and runs on the device
 *   1. the reversible path: level shift, RCT, int16 CDF 5/3 forward and inverse -- the pixels must come back identical;
 *   2. the irreversible path: level shift, scale 1/256, ICT, float CDF 9/7 on binary16 storage -- prints the largest
 *      pixel error.
 * Own code written against include/libdwt_hip.h.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/picture_lossless.c -o picture_lossless \
 *       -Llibdwt_amd -l:libdwt_hip.so -Wl,-rpath,$PWD/libdwt_amd -lm
 *   ./picture_lossless [picture.ppm]
 */
#include "libdwt.h"
#include "libdwt_hip.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* the next decimal number of a PPM header: white space and # comments skipped; -1 at the end of the file */
static int ppm_number(FILE *f)
{
	int c = fgetc(f);
	while (c == '#' || c == ' ' || c == '\t' || c == '\n' || c == '\r') {
		if (c == '#')
			while (c != '\n' && c != EOF)
				c = fgetc(f);
		else
			c = fgetc(f);
	}
	if (c < '0' || c > '9')
		return -1;
	int v = 0;
	while (c >= '0' && c <= '9' && v < 100000000) {
		v = 10 * v + (c - '0');
		c = fgetc(f);
	}
	return v; /* (the one white-space byte after the number is consumed, as the format wants after maxval) */
}

static unsigned char *ppm_read(const char *path, int *w, int *h)
{
	FILE *f = fopen(path, "rb");
	if (!f)
		return NULL;
	unsigned char *pix = NULL;
	if (fgetc(f) == 'P' && fgetc(f) == '6') {
		*w = ppm_number(f);
		*h = ppm_number(f);
		const int maxval = ppm_number(f);
		if (*w > 0 && *h > 0 && *w <= 32768 && *h <= 32768 && maxval == 255) {
			const size_t n = (size_t)*w * *h * 3;
			pix = malloc(n);
			if (pix && fread(pix, 1, n, f) != n) {
				free(pix);
				pix = NULL;
			}
		}
	}
	fclose(f);
	return pix;
}

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

int main(int argc, char **argv)
{
	dwt_util_init();
	dwt_util_log(LOG_INFO, "library: %s on %s\n", dwt_util_version(), dwt_hip_device_name());

	int w = 640, h = 480;
	unsigned char *pix = argc > 1 ? ppm_read(argv[1], &w, &h) : synthetic(w, h);
	if (!pix)
		dwt_util_error("no picture: %s is not a binary PPM with maxval 255\n", argc > 1 ? argv[1] : "(synthetic)");
	const size_t n = (size_t)w * h * 3, row = (size_t)w * 3, plane_pitch = (size_t)w * 2, plane = plane_pitch * h;
	unsigned char *back = malloc(n);
	void *d_pix = dwt_hip_malloc(n), *d_back = dwt_hip_malloc(n), *d_planes = dwt_hip_malloc(3 * plane);
	if (!back || !d_pix || !d_back || !d_planes)
		dwt_util_error("allocation failed: %s\n", dwt_hip_last_error());
	dwt_hip_memcpy_h2d(d_pix, pix, n); /* the 8-bit pixels cross once; nothing is widened on the host */

	/* 1. reversible */
	int j = -1;
	if (dwt_hip_picture_forward_batch(DWT_HIP_CDF53_I16, DWT_HIP_PIX_U8, d_pix, n, row, 3, 1, 1, 3, DWT_HIP_ORDER_RGB, 8, 128, 1.0f,
			DWT_HIP_COLOUR_RCT, d_planes, plane, plane_pitch, w, h, &j) ||
	    dwt_hip_picture_inverse_batch(DWT_HIP_CDF53_I16, DWT_HIP_PIX_U8, d_back, n, row, 3, 1, 1, 3, DWT_HIP_ORDER_RGB, 8, 128, 1.0f,
			DWT_HIP_COLOUR_RCT, d_planes, plane, plane_pitch, w, h, j))
		dwt_util_error("reversible path: %s\n", dwt_hip_last_error());
	dwt_hip_memcpy_d2h(back, d_back, n);
	const int identical = memcmp(pix, back, n) == 0;
	printf("%d x %d RGB8, RCT + int16 CDF 5/3, %d levels: pixels %s\n", w, h, j, identical ? "identical" : "DIFFER");

	/* 2. irreversible: samples in [-0.5, 0.5) on binary16 storage */
	j = 5;
	if (dwt_hip_picture_forward_batch(DWT_HIP_CDF97_H, DWT_HIP_PIX_U8, d_pix, n, row, 3, 1, 1, 3, DWT_HIP_ORDER_RGB, 8, 128, 1.0f / 256,
			DWT_HIP_COLOUR_ICT, d_planes, plane, plane_pitch, w, h, &j) ||
	    dwt_hip_picture_inverse_batch(DWT_HIP_CDF97_H, DWT_HIP_PIX_U8, d_back, n, row, 3, 1, 1, 3, DWT_HIP_ORDER_RGB, 8, 128, 256.0f,
			DWT_HIP_COLOUR_ICT, d_planes, plane, plane_pitch, w, h, j))
		dwt_util_error("irreversible path: %s\n", dwt_hip_last_error());
	dwt_hip_memcpy_d2h(back, d_back, n);
	int err = 0;
	for (size_t i = 0; i < n; i++) {
		const int e = abs((int)back[i] - (int)pix[i]);
		err = e > err ? e : err;
	}
	printf("%d x %d RGB8, ICT + float CDF 9/7 on binary16, %d levels: largest pixel error %d of 255\n", w, h, j, err);

	dwt_hip_free(d_pix);
	dwt_hip_free(d_back);
	dwt_hip_free(d_planes);
	free(pix);
	free(back);
	dwt_util_finish();
	return identical ? 0 : 1;
}
