/*
 * swt_denoise.c -- translation-invariant denoising of a small batch of images that stays resident in device memory: noise
 * of a known sigma is added to smooth test images, the batch goes through the stationary CDF 9/7 transform under the
 * symmetric border (dwt_hip_swt2d_batch_ex) and comes back through dwt_hip_iswt2d_batch with a SOFT table of the universal
 * threshold sigma * sqrt(2 ln n) on the two finest levels -- the shrinkage is applied as the inverse reads the
 * coefficients, so the planes are passed over once.  Prints the PSNR before and after, and the error of the plain round
 * trip (no table) relative to max|x|.  The images are computed, the noise is seeded; no input file is read.  Own code
 * written against include/.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/swt_denoise.c -o swt_denoise -Llibdwt_amd -l:libdwt_hip.so -Wl,-rpath,$PWD/libdwt_amd -lm
 */
#include "libdwt.h"
#include "libdwt_hip.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>

static double uniform(unsigned *s) /* a small LCG, in (0, 1) */
{
	*s = *s * 1664525u + 1013904223u;
	return ((*s >> 8) + 0.5) / 16777216.0;
}

static double gauss(unsigned *s) /* Box-Muller */
{
	const double u = uniform(s), v = uniform(s);
	return sqrt(-2.0 * log(u)) * cos(6.283185307179586 * v);
}

static double psnr(const float *a, const float *b, size_t n, double peak)
{
	double se = 0;
	for (size_t i = 0; i < n; i++)
		se += ((double)a[i] - b[i]) * ((double)a[i] - b[i]);
	return 10.0 * log10(peak * peak * (double)n / se);
}

int main(void)
{
	dwt_util_init();
	dwt_util_log(LOG_INFO, "library: %s on %s\n", dwt_util_version(), dwt_hip_device_name());

	enum { batch = 2, size_x = 200, size_y = 144, levels = 4, shrunk = 2 };
	const float sigma = 0.1f;
	const size_t plane = (size_t)size_x * size_y, plane_bytes = plane * sizeof(float), n = batch * plane;
	enum { per_image = 3 * levels + 1 }; /* HL, LH, HH of every level, then the last level's LL */
	float *clean = malloc(n * sizeof(float)), *noisy = malloc(n * sizeof(float)), *back = malloc(n * sizeof(float));
	unsigned seed = 2025;
	for (int b = 0; b < batch; b++)
		for (int y = 0; y < size_y; y++)
			for (int x = 0; x < size_x; x++) {
				const size_t i = ((size_t)b * size_y + y) * size_x + x;
				/* smooth waves and one edge, in [-1, 1] */
				clean[i] = (float)(0.5 * sin(x / 17.0 + b) * cos(y / 23.0) + (x + 2 * y > size_x ? 0.4 : -0.4));
				noisy[i] = clean[i] + sigma * (float)gauss(&seed);
			}

	float *d_img = dwt_hip_malloc(n * sizeof(float)), *d_coef = dwt_hip_malloc((size_t)batch * per_image * plane_bytes),
	      *d_back = dwt_hip_malloc(n * sizeof(float));
	if (!d_img || !d_coef || !d_back || dwt_hip_memcpy_h2d(d_img, noisy, n * sizeof(float)))
		dwt_util_error("device setup: %s\n", dwt_hip_last_error());
	const size_t pitch = size_x * sizeof(float);
	float *const d_ll = d_coef + 3 * levels * plane; /* the last LL behind every image's detail planes */
	if (dwt_hip_swt2d_batch_ex(DWT_HIP_CDF97_S, d_img, plane_bytes, batch, (int)pitch, sizeof(float), size_x, size_y, levels, d_coef, d_ll, 1,
		    per_image * plane_bytes, plane_bytes, (int)pitch, DWT_HIP_SWT_BORDER_SYMMETRIC))
		dwt_util_error("dwt_hip_swt2d_batch_ex: %s\n", dwt_hip_last_error());

	/* the universal threshold on the finest levels, the coarser ones kept */
	int ops[3 * levels];
	float params[3 * levels];
	for (int i = 0; i < 3 * levels; i++) {
		ops[i] = i < 3 * shrunk ? DWT_HIP_BAND_SOFT : DWT_HIP_BAND_KEEP;
		params[i] = i < 3 * shrunk ? sigma * sqrtf(2.f * logf((float)plane)) : 0.f;
	}
	if (dwt_hip_iswt2d_batch(DWT_HIP_CDF97_S, DWT_HIP_SWT_BORDER_SYMMETRIC, d_coef, d_ll, per_image * plane_bytes, plane_bytes, (int)pitch, batch,
		    size_x, size_y, levels, ops, params, d_back, plane_bytes, (int)pitch, sizeof(float)) ||
		dwt_hip_memcpy_d2h(back, d_back, n * sizeof(float)))
		dwt_util_error("dwt_hip_iswt2d_batch: %s\n", dwt_hip_last_error());
	printf("PSNR noisy (dB): %.2f\n", psnr(clean, noisy, n, 2.0));
	printf("PSNR denoised (dB): %.2f\n", psnr(clean, back, n, 2.0));

	/* the plain round trip: no table */
	if (dwt_hip_iswt2d_batch(DWT_HIP_CDF97_S, DWT_HIP_SWT_BORDER_SYMMETRIC, d_coef, d_ll, per_image * plane_bytes, plane_bytes, (int)pitch, batch,
		    size_x, size_y, levels, NULL, NULL, d_back, plane_bytes, (int)pitch, sizeof(float)) ||
		dwt_hip_memcpy_d2h(back, d_back, n * sizeof(float)))
		dwt_util_error("dwt_hip_iswt2d_batch: %s\n", dwt_hip_last_error());
	double err = 0, top = 0;
	for (size_t i = 0; i < n; i++) {
		err = fmax(err, fabs((double)back[i] - noisy[i]));
		top = fmax(top, fabs((double)noisy[i]));
	}
	printf("round trip max error / max|x|: %.3g\n", err / top);

	dwt_hip_free(d_img);
	dwt_hip_free(d_coef);
	dwt_hip_free(d_back);
	free(clean), free(noisy), free(back);
	dwt_util_finish();
	return 0;
}
