/*
 * picture_embedded.c -- a colour picture through the irreversible path, its indices crossing to the host and back as an
 * embedded bit-plane stream of code-blocks (an extension of this library).  Fills a synthetic RGB8 picture,
 * or reads a binary PPM (P6, maxval 255), uploads the bytes once and runs on the device
 *   dwt_hip_picture_forward_batch   level shift, ICT, float CDF 9/7, 5 levels
 *   dwt_hip_quantize_batch          deadzone quantizer to int16 indices
 *   dwt_hip_bitplane_pack_batch     count only (the sizing call), then the words of every 64 x 64 code-block
 * The words and the offsets ALONE go down to the host and up again.  Then, for drop = 0, 1, 2, 3,
 *   dwt_hip_bitplane_unpack_batch   the planes but the `drop` least significant ones, mode SHIFT
 *   dwt_hip_dequantize_batch        with the steps times 2^drop, r = 0.5
 *   dwt_hip_picture_inverse_batch   back to pixels
 * and prints, per drop, the bytes a receiver of that quality needs against the bytes of the int16 planes, and the PSNR.
 * At drop 0 the PSNR is that of the flow without the detour (the first line; examples/picture_lossy.c at this base step), to
 * the last digit: the indices come back bit for bit.  Own code written against include/libdwt_hip.h.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/picture_embedded.c -o picture_embedded \
 *       -Llibdwt_amd -l:libdwt_hip.so -Wl,-rpath,$PWD/libdwt_amd -lm
 *   ./picture_embedded [picture.ppm]
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
	unsigned char *back = malloc(n);
	void *d_pix = dwt_hip_malloc(n), *d_back = dwt_hip_malloc(n), *d_coef = dwt_hip_malloc(3 * coef_plane), *d_index = dwt_hip_malloc(3 * index_plane);
	if (!back || !d_pix || !d_back || !d_coef || !d_index)
		dwt_util_error("allocation failed: %s\n", dwt_hip_last_error());
	dwt_hip_memcpy_h2d(d_pix, pix, n); /* the 8-bit pixels cross once; nothing is widened on the host */

	/* ---- forward, quantize: the three planes Y, Cb, Cr are a batch of three frames with one table */
	const float base = 2.0f;
	float steps[DWT_HIP_BAND_MAX_SLOTS], coarse[DWT_HIP_BAND_MAX_SLOTS];
	int j = 5;
	if (dwt_hip_picture_forward_batch(DWT_HIP_CDF97_S, DWT_HIP_PIX_U8, d_pix, n, row, 3, 1, 1, 3, DWT_HIP_ORDER_RGB, 8, 128, 1.0f, DWT_HIP_COLOUR_ICT,
			d_coef, coef_plane, coef_pitch, w, h, &j) ||
	    dwt_hip_quant_steps(DWT_HIP_CDF97_S, j, base, steps) ||
	    dwt_hip_quantize_batch(DWT_HIP_COEF_S, d_coef, coef_plane, coef_pitch, DWT_HIP_INDEX_I16, d_index, index_plane, index_pitch, 3, w, h, j, steps,
			0, NULL))
		dwt_util_error("forward: %s\n", dwt_hip_last_error());
	const int slots = dwt_hip_band_slots(j);

	/* ---- the flow without the detour */
	if (dwt_hip_dequantize_batch(DWT_HIP_INDEX_I16, d_index, index_plane, index_pitch, DWT_HIP_COEF_S, d_coef, coef_plane, coef_pitch, 3, w, h, j, steps, 0,
			0.5f) ||
	    dwt_hip_picture_inverse_batch(DWT_HIP_CDF97_S, DWT_HIP_PIX_U8, d_back, n, row, 3, 1, 1, 3, DWT_HIP_ORDER_RGB, 8, 128, 1.0f, DWT_HIP_COLOUR_ICT,
			d_coef, coef_plane, coef_pitch, w, h, j))
		dwt_util_error("direct path: %s\n", dwt_hip_last_error());
	dwt_hip_memcpy_d2h(back, d_back, n);
	const double direct = psnr_of(back, pix, n);
	printf("%d x %d RGB8, %d levels, base step %.1f, the indices left on the device: PSNR %.6f dB\n", w, h, j, (double)base, direct);

	/* ---- count, pack */
	int table[5 * (DWT_HIP_BAND_MAX_SLOTS + 1)];
	const int bands = dwt_hip_bitplane_bands(w, h, j, 6, 6, table);
	if (bands < 0)
		dwt_util_error("bit-plane bands refused %d x %d\n", w, h);
	const int S = table[5 * bands + 4];
	unsigned *off = malloc(3 * (size_t)(S + 1) * sizeof *off);
	if (!off || dwt_hip_bitplane_pack_batch(DWT_HIP_INDEX_I16, d_index, index_plane, index_pitch, 3, w, h, j, 6, 6, NULL, 0, off))
		dwt_util_error("count: %s\n", dwt_hip_last_error());
	size_t cap = 1;
	for (int b = 0; b < 3; b++)
		cap = off[b * (S + 1) + S] > cap ? off[b * (S + 1) + S] : cap;
	uint64_t *words = malloc(3 * cap * sizeof *words);
	uint64_t *d_words = dwt_hip_malloc(3 * cap * sizeof *words);
	unsigned *d_off = dwt_hip_malloc(3 * (size_t)(S + 1) * sizeof *off);
	if (!words || !d_words || !d_off ||
	    dwt_hip_bitplane_pack_batch(DWT_HIP_INDEX_I16, d_index, index_plane, index_pitch, 3, w, h, j, 6, 6, d_words, cap, d_off))
		dwt_util_error("pack: %s\n", dwt_hip_last_error());

	/* ---- the words and the offsets alone go down and up again: the planes are forgotten on the way */
	dwt_hip_memcpy_d2h(words, d_words, 3 * cap * sizeof *words);
	dwt_hip_memcpy_d2h(off, d_off, 3 * (size_t)(S + 1) * sizeof *off);
	dwt_hip_free(d_words);
	dwt_hip_free(d_off);
	dwt_hip_free(d_index);
	d_words = dwt_hip_malloc(3 * cap * sizeof *words);
	d_off = dwt_hip_malloc(3 * (size_t)(S + 1) * sizeof *off);
	d_index = dwt_hip_malloc(3 * index_plane);
	if (!d_words || !d_off || !d_index)
		dwt_util_error("allocation failed: %s\n", dwt_hip_last_error());
	dwt_hip_memcpy_h2d(d_words, words, 3 * cap * sizeof *words);
	dwt_hip_memcpy_h2d(d_off, off, 3 * (size_t)(S + 1) * sizeof *off);

	/* ---- unpack at four qualities */
	int ok = 1;
	for (int drop = 0; drop <= 3; drop++) {
		/* what a receiver of this quality needs: of every block its planes but the `drop` least significant ones */
		unsigned long long crossed = 0;
		for (int b = 0; b < 3; b++)
			for (int s = 0; s < S; s++) {
				int x, y, cw, ch;
				if (dwt_hip_bitplane_block(table, bands, 6, 6, s, &x, &y, &cw, &ch))
					dwt_util_error("block %d\n", s);
				const unsigned G = ((unsigned)(cw * ch) + 63) / 64, len = off[b * (S + 1) + s + 1] - off[b * (S + 1) + s];
				const unsigned p = len ? len / G - 1 : 0, kept = p > (unsigned)drop ? p - drop : 0;
				crossed += kept ? 8ull * (kept + 1) * G : 0;
			}
		crossed += 3ull * (S + 1) * sizeof *off;
		for (int k = 0; k < slots; k++)
			coarse[k] = steps[k] * (float)(1 << drop);
		if (dwt_hip_bitplane_unpack_batch(DWT_HIP_INDEX_I16, d_words, cap, d_off, d_index, index_plane, index_pitch, 3, w, h, j, 6, 6, drop,
				DWT_HIP_BITPLANE_SHIFT) ||
		    dwt_hip_dequantize_batch(DWT_HIP_INDEX_I16, d_index, index_plane, index_pitch, DWT_HIP_COEF_S, d_coef, coef_plane, coef_pitch, 3, w, h, j,
				coarse, 0, 0.5f) ||
		    dwt_hip_picture_inverse_batch(DWT_HIP_CDF97_S, DWT_HIP_PIX_U8, d_back, n, row, 3, 1, 1, 3, DWT_HIP_ORDER_RGB, 8, 128, 1.0f,
				DWT_HIP_COLOUR_ICT, d_coef, coef_plane, coef_pitch, w, h, j))
			dwt_util_error("embedded path: %s\n", dwt_hip_last_error());
		dwt_hip_memcpy_d2h(back, d_back, n);
		const double psnr = psnr_of(back, pix, n);
		printf("drop %d (step x %d): %llu bytes of words and offsets against %zu bytes of int16 planes (%.1f %%, %.2f bit / sample), PSNR %.6f dB\n",
			drop, 1 << drop, crossed, 3 * index_plane, 100.0 * (double)crossed / (double)(3 * index_plane),
			8.0 * (double)crossed / ((double)w * h * 3), psnr);
		if (drop == 0)
			ok = ok && psnr == direct; /* the same indices: the same pixels */
		ok = ok && psnr > 15.0 && crossed < 3 * index_plane;
	}

	dwt_hip_free(d_pix);
	dwt_hip_free(d_back);
	dwt_hip_free(d_coef);
	dwt_hip_free(d_index);
	dwt_hip_free(d_words);
	dwt_hip_free(d_off);
	free(pix);
	free(back);
	free(words);
	free(off);
	dwt_util_finish();
	return ok ? 0 : 1;
}
