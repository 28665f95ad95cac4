/*
 * picture_sparse.c -- a colour picture through the irreversible path down to integer indices, the indices across PCIe as
 * sparse streams, and back (an extension of this library).  Fills a synthetic RGB8 picture, or reads a binary
 * PPM (P6, maxval 255), uploads the bytes once and runs on the device
 *   dwt_hip_picture_forward_batch   level shift, ICT, float CDF 9/7, 5 levels
 *   dwt_hip_quantize_batch          deadzone quantizer to int16 indices
 *   dwt_hip_sparse_pack_batch       count only (the sizing call), then the (position, value) entries in resolution order
 *   -- only the streams cross PCIe, down and up again: what a coder, a store or a peer would take and give --
 *   dwt_hip_sparse_unpack_batch     the index planes again
 *   dwt_hip_dequantize_batch        reconstruction at r = 0.5
 *   dwt_hip_picture_inverse_batch   back to pixels
 * and prints the bytes that crossed against the bytes of the index planes, and the PSNR with and without the detour: the two
 * must agree to the last digit printed (the pictures are in fact the same bytes).  Own code written against
 * include/libdwt_hip.h.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/picture_sparse.c -o picture_sparse \
 *       -Llibdwt_amd -l:libdwt_hip.so -Wl,-rpath,$PWD/libdwt_amd -lm
 *   ./picture_sparse [picture.ppm]
 */
#include "libdwt.h"
#include "libdwt_hip.h"

#include <math.h>
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

static double psnr_of(const unsigned char *a, const unsigned char *b, size_t n)
{
	double sq = 0;
	for (size_t i = 0; i < n; i++) {
		const double e = (double)a[i] - (double)b[i];
		sq += e * e;
	}
	return sq > 0 ? 10.0 * log10(255.0 * 255.0 * (double)n / sq) : INFINITY;
}

int main(int argc, char **argv)
{
	dwt_util_init();
	dwt_util_log(LOG_INFO, "library: %s on %s\n", dwt_util_version(), dwt_hip_device_name());

	int w = 640, h = 480;
	unsigned char *pix = argc > 1 ? ppm_read(argv[1], &w, &h) : synthetic(w, h);
	if (!pix)
		dwt_util_error("no picture: %s is not a binary PPM with maxval 255\n", argc > 1 ? argv[1] : "(synthetic)");
	const size_t n = (size_t)w * h * 3, row = (size_t)w * 3;
	const size_t coef_pitch = (size_t)w * 4, coef_plane = coef_pitch * h, index_pitch = (size_t)w * 2, index_plane = index_pitch * h;
	unsigned char *back = malloc(n), *back_direct = malloc(n);
	void *d_pix = dwt_hip_malloc(n), *d_back = dwt_hip_malloc(n), *d_coef = dwt_hip_malloc(3 * coef_plane), *d_index = dwt_hip_malloc(3 * index_plane),
	     *d_index2 = dwt_hip_malloc(3 * index_plane);
	if (!back || !back_direct || !d_pix || !d_back || !d_coef || !d_index || !d_index2)
		dwt_util_error("allocation failed: %s\n", dwt_hip_last_error());
	dwt_hip_memcpy_h2d(d_pix, pix, n); /* the 8-bit pixels cross once; nothing is widened on the host */

	/* ---- forward and quantize: the three planes Y, Cb, Cr are a batch of three frames with one table */
	float steps[DWT_HIP_BAND_MAX_SLOTS];
	int j = 5;
	if (dwt_hip_picture_forward_batch(DWT_HIP_CDF97_S, DWT_HIP_PIX_U8, d_pix, n, row, 3, 1, 1, 3, DWT_HIP_ORDER_RGB, 8, 128, 1.0f,
			DWT_HIP_COLOUR_ICT, d_coef, coef_plane, coef_pitch, w, h, &j) ||
	    dwt_hip_quant_steps(DWT_HIP_CDF97_S, j, 2.0f, steps) ||
	    dwt_hip_quantize_batch(DWT_HIP_COEF_S, d_coef, coef_plane, coef_pitch, DWT_HIP_INDEX_I16, d_index, index_plane, index_pitch, 3, w, h, j, steps,
			0, NULL))
		dwt_util_error("forward path: %s\n", dwt_hip_last_error());
	const int words = dwt_hip_band_slots(j) + 1; /* offsets of a frame: one per band, and the total */

	/* ---- count, then pack: the offsets tell the capacity */
	unsigned off[3 * (DWT_HIP_BAND_MAX_SLOTS + 1)];
	if (dwt_hip_sparse_pack_batch(DWT_HIP_SPARSE_I16, d_index, index_plane, index_pitch, 3, w, h, j, NULL, NULL, 0, off))
		dwt_util_error("count: %s\n", dwt_hip_last_error());
	size_t cap = 1, entries = 0;
	for (int b = 0; b < 3; b++) {
		const unsigned total = off[b * words + words - 1];
		cap = total > cap ? total : cap;
		entries += total;
	}
	unsigned *d_pos = dwt_hip_malloc(3 * cap * 4), *d_off = dwt_hip_malloc(3 * (size_t)words * 4);
	short *d_val = dwt_hip_malloc(3 * cap * 2);
	unsigned *pos = malloc(3 * cap * 4);
	short *val = malloc(3 * cap * 2);
	if (!d_pos || !d_val || !d_off || !pos || !val)
		dwt_util_error("allocation failed: %s\n", dwt_hip_last_error());
	if (dwt_hip_sparse_pack_batch(DWT_HIP_SPARSE_I16, d_index, index_plane, index_pitch, 3, w, h, j, d_pos, d_val, cap, d_off))
		dwt_util_error("pack: %s\n", dwt_hip_last_error());

	/* ---- only the streams cross: every frame's entries and its offsets, down ... */
	size_t crossed = 0;
	for (int b = 0; b < 3; b++) {
		const size_t total = off[b * words + words - 1];
		if (total) {
			dwt_hip_memcpy_d2h(pos + b * cap, d_pos + b * cap, total * 4);
			dwt_hip_memcpy_d2h(val + b * cap, d_val + b * cap, total * 2);
		}
		crossed += total * 6;
	}
	dwt_hip_memcpy_d2h(off, d_off, 3 * (size_t)words * 4);
	crossed += 3 * (size_t)words * 4;
	/* ... (here a coder would take them: a prefix of a frame's stream, cut at off[k], is a coarser picture) ... and up again,
	 * into buffers that held something else */
	dwt_hip_memcpy_h2d(d_index2, pix, n < 3 * index_plane ? n : 3 * index_plane);
	for (int b = 0; b < 3; b++) {
		const size_t total = off[b * words + words - 1];
		if (total) {
			dwt_hip_memcpy_h2d(d_pos + b * cap, pos + b * cap, total * 4);
			dwt_hip_memcpy_h2d(d_val + b * cap, val + b * cap, total * 2);
		}
	}
	dwt_hip_memcpy_h2d(d_off, off, 3 * (size_t)words * 4);

	/* ---- unpack, dequantize, inverse; and the same without the detour */
	if (dwt_hip_sparse_unpack_batch(DWT_HIP_SPARSE_I16, d_pos, d_val, cap, d_off + words - 1, (size_t)words, d_index2, index_plane, index_pitch, 3, w, h))
		dwt_util_error("unpack: %s\n", dwt_hip_last_error());
	const void *index_of[2] = {d_index2, d_index};
	unsigned char *back_of[2] = {back, back_direct};
	for (int k = 0; k < 2; k++) {
		if (dwt_hip_dequantize_batch(DWT_HIP_INDEX_I16, index_of[k], index_plane, index_pitch, DWT_HIP_COEF_S, d_coef, coef_plane, coef_pitch, 3, w, h, j,
				steps, 0, 0.5f) ||
		    dwt_hip_picture_inverse_batch(DWT_HIP_CDF97_S, DWT_HIP_PIX_U8, d_back, n, row, 3, 1, 1, 3, DWT_HIP_ORDER_RGB, 8, 128, 1.0f,
				DWT_HIP_COLOUR_ICT, d_coef, coef_plane, coef_pitch, w, h, j))
			dwt_util_error("inverse path: %s\n", dwt_hip_last_error());
		dwt_hip_memcpy_d2h(back_of[k], d_back, n);
	}
	char through[64], direct[64];
	snprintf(through, sizeof through, "%.4f", psnr_of(back, pix, n));
	snprintf(direct, sizeof direct, "%.4f", psnr_of(back_direct, pix, n));
	printf("%d x %d RGB8, %d levels, base step 2.0: %zu entries of %zu indices (%.2f %%)\n", w, h, j, entries, (size_t)w * h * 3,
		100.0 * (double)entries / ((double)w * h * 3));
	printf("crossed PCIe each way: %zu bytes of streams and offsets, against %zu bytes of index planes (%.1f %%)\n", crossed, 3 * index_plane,
		100.0 * (double)crossed / (double)(3 * index_plane));
	printf("through the streams: PSNR %s dB\nwithout the detour:  PSNR %s dB\n", through, direct);
	const int ok = strcmp(through, direct) == 0 && memcmp(back, back_direct, n) == 0;
	if (!ok)
		printf("the detour changed the picture\n");

	dwt_hip_free(d_pix);
	dwt_hip_free(d_back);
	dwt_hip_free(d_coef);
	dwt_hip_free(d_index);
	dwt_hip_free(d_index2);
	dwt_hip_free(d_pos);
	dwt_hip_free(d_val);
	dwt_hip_free(d_off);
	free(pix);
	free(back);
	free(back_direct);
	free(pos);
	free(val);
	dwt_util_finish();
	return ok ? 0 : 1;
}
