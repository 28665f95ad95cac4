/*
 * picture_lossy.c -- a colour picture through the irreversible path down to integer indices and back (an
 * extension of this library).  Fills a synthetic RGB8 picture, or reads a binary PPM (P6, maxval 255), uploads the bytes
 * once and runs on the device, for three base steps,
 *   dwt_hip_picture_forward_batch   level shift, ICT, float CDF 9/7, 5 levels
 *   dwt_hip_quant_steps             one step per subband: the base step over the band's synthesis norm
 *   dwt_hip_quantize_batch          deadzone quantizer to int16 indices, with the per-band counters
 *   dwt_hip_codeblock_bitplanes_batch   the magnitude bit-planes of every 64 x 64 code-block
 *   dwt_hip_dequantize_batch        reconstruction at r = 0.5
 *   dwt_hip_picture_inverse_batch   back to pixels
 * and prints the PSNR, the share of nonzero indices, the clipped samples and the bit-planes a coder would have to code.
 * Only the pixels and the small tables cross PCIe.  Own code written against include/libdwt_hip.h.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/picture_lossy.c -o picture_lossy \
 *       -Llibdwt_amd -l:libdwt_hip.so -Wl,-rpath,$PWD/libdwt_amd -lm
 *   ./picture_lossy [picture.ppm]
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

	int first[DWT_HIP_BAND_MAX_SLOTS + 1];
	long long stats[3 * 3 * DWT_HIP_BAND_MAX_SLOTS];
	float steps[DWT_HIP_BAND_MAX_SLOTS];
	const float base[3] = {0.5f, 2.0f, 8.0f};
	int ok = 1;
	for (int k = 0; k < 3; k++) {
		int j = 5;
		if (dwt_hip_picture_forward_batch(DWT_HIP_CDF97_S, DWT_HIP_PIX_U8, d_pix, n, row, 3, 1, 1, 3, DWT_HIP_ORDER_RGB, 8, 128, 1.0f,
				DWT_HIP_COLOUR_ICT, d_coef, coef_plane, coef_pitch, w, h, &j))
			dwt_util_error("forward: %s\n", dwt_hip_last_error());
		const int slots = dwt_hip_band_slots(j);
		const int blocks = dwt_hip_codeblock_layout(w, h, j, 6, 6, first, NULL);
		unsigned char *planes = blocks > 0 ? malloc(3 * (size_t)blocks) : NULL;
		if (blocks < 0 || !planes)
			dwt_util_error("code-blocks: %s\n", dwt_hip_last_error());
		/* the three planes Y, Cb, Cr are a batch of three frames with one table */
		if (dwt_hip_quant_steps(DWT_HIP_CDF97_S, j, base[k], steps) ||
		    dwt_hip_quantize_batch(DWT_HIP_COEF_S, d_coef, coef_plane, coef_pitch, DWT_HIP_INDEX_I16, d_index, index_plane, index_pitch, 3, w, h, j,
				steps, 0, stats) ||
		    dwt_hip_codeblock_bitplanes_batch(DWT_HIP_INDEX_I16, d_index, index_plane, index_pitch, 3, w, h, j, 6, 6, planes, (size_t)blocks) ||
		    dwt_hip_dequantize_batch(DWT_HIP_INDEX_I16, d_index, index_plane, index_pitch, DWT_HIP_COEF_S, d_coef, coef_plane, coef_pitch, 3, w, h, j,
				steps, 0, 0.5f) ||
		    dwt_hip_picture_inverse_batch(DWT_HIP_CDF97_S, DWT_HIP_PIX_U8, d_back, n, row, 3, 1, 1, 3, DWT_HIP_ORDER_RGB, 8, 128, 1.0f,
				DWT_HIP_COLOUR_ICT, d_coef, coef_plane, coef_pitch, w, h, j))
			dwt_util_error("lossy path: %s\n", dwt_hip_last_error());
		dwt_hip_memcpy_d2h(back, d_back, n);
		double sq = 0;
		for (size_t i = 0; i < n; i++) {
			const double e = (double)back[i] - (double)pix[i];
			sq += e * e;
		}
		const double psnr = sq > 0 ? 10.0 * log10(255.0 * 255.0 * (double)n / sq) : INFINITY;
		long long nonzero = 0, clipped = 0, top = 0, coded = 0;
		for (int i = 0; i < 3 * slots; i++) {
			nonzero += stats[3 * i];
			top = stats[3 * i + 1] > top ? stats[3 * i + 1] : top;
			clipped += stats[3 * i + 2];
		}
		for (int i = 0; i < 3 * blocks; i++)
			coded += planes[i];
		printf("%d x %d RGB8, %d levels, base step %4.1f: PSNR %6.2f dB, %5.2f %% of the indices nonzero, largest magnitude %lld, "
		       "%lld clipped, %.2f bit-planes per 64 x 64 code-block (%d blocks)\n",
			w, h, j, (double)base[k], psnr, 100.0 * (double)nonzero / ((double)w * h * 3), top, clipped, (double)coded / (3.0 * blocks), 3 * blocks);
		ok = ok && clipped == 0 && psnr > 20.0;
		free(planes);
	}

	dwt_hip_free(d_pix);
	dwt_hip_free(d_back);
	dwt_hip_free(d_coef);
	dwt_hip_free(d_index);
	free(pix);
	free(back);
	dwt_util_finish();
	return ok ? 0 : 1;
}
