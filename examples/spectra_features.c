/*
 * spectra_features.c -- the flow of libdwt's examples/spectra-dwt on synthetic rows: a matrix of spectra (one per
 * row) is transformed row-wise with dwt_cdf97_2f1_s, then every row's wavelet power spectrum is taken with
 * dwt_util_wps_s (size_y = 1), which gives the feature matrix a classifier is fed with.  Here the same matrix also
 * comes from ONE batch call, dwt_hip_features1d_batch, and both must agree bit for bit -- on host rows, and on rows
 * resident in device memory, where the coefficients never leave the device: the only download is the feature matrix.
 * The rows are seeded noise over a few smooth lines; no input file is read.  Own code written against include/libdwt.h.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/spectra_features.c -o spectra_features \
 *       -Llibdwt_amd -l:libdwt_hip.so -Wl,-rpath,$PWD/libdwt_amd -lm
 */
#include "libdwt.h"
#include "libdwt_hip.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

static unsigned rnd(unsigned *s) /* a small LCG: the same rows everywhere */
{
	*s = *s * 1664525u + 1013904223u;
	return *s >> 8;
}

int main(void)
{
	dwt_util_init();
	dwt_util_log(LOG_INFO, "library: %s on %s\n", dwt_util_version(), dwt_hip_device_name());

	const int rows = 256, n = 4096;
	const int stride_y = sizeof(float), stride_x = n * stride_y;
	const size_t bytes = (size_t)rows * stride_x;
	float *spectra = malloc(bytes), *coeffs = malloc(bytes);
	unsigned seed = 12345;
	for (int y = 0; y < rows; y++) {
		const float centre = (float)(rnd(&seed) % n), width = 20.f + (float)(rnd(&seed) % 200);
		for (int x = 0; x < n; x++) {
			const float t = ((float)x - centre) / width;
			spectra[(size_t)y * n + x] = 1.f - 0.6f * expf(-t * t) + ((float)(rnd(&seed) & 0xffff) / 65536.f - 0.5f) * 0.05f;
		}
	}

	/* host rows: transform, then the reference's loop over rows against the batch call */
	memcpy(coeffs, spectra, bytes);
	int j = -1;
	dwt_cdf97_2f1_s(coeffs, stride_x, stride_y, n, rows, n, rows, &j, 0);
	const int j_max = j + 1; /* the vectors visit levels 1 .. j_max-1 */
	const int count = dwt_util_count_subbands_s(coeffs, stride_x, stride_y, n, 1, n, 1, j_max);
	dwt_util_log(LOG_INFO, "%d rows of %d samples, %d levels, %d features per row\n", rows, n, j, count);
	float *by_row = malloc((size_t)rows * count * sizeof(float)), *by_batch = malloc((size_t)rows * count * sizeof(float));
	for (int y = 0; y < rows; y++)
		dwt_util_wps_s(coeffs + (size_t)y * n, stride_x, stride_y, n, 1, n, 1, j_max, by_row + (size_t)y * count);
	if (dwt_hip_features1d_batch(DWT_HIP_FEATURE_BIT(DWT_HIP_FEATURE_WPS), coeffs, stride_x, stride_y, rows, n, j_max, 2.f, by_batch, count))
		dwt_util_error("batch call: %s\n", dwt_hip_last_error());
	const int bad_host = memcmp(by_row, by_batch, (size_t)rows * count * sizeof(float)) != 0;
	dwt_util_log(LOG_INFO, bad_host ? "host rows: per-row and batch features differ\n" : "host rows: success\n");

	/* device-resident rows: uploaded once, transformed and reduced in place; one download, the feature matrix */
	float *d = dwt_hip_malloc(bytes), *dfv = dwt_hip_malloc((size_t)rows * count * sizeof(float));
	float *from_device = malloc((size_t)rows * count * sizeof(float)), *row_fv = malloc(count * sizeof(float));
	if (!d || !dfv || dwt_hip_memcpy_h2d(d, spectra, bytes))
		dwt_util_error("device setup: %s\n", dwt_hip_last_error());
	int jd = -1;
	dwt_cdf97_2f1_s(d, stride_x, stride_y, n, rows, n, rows, &jd, 0);
	const int launches0 = dwt_hip_get_option("stat_launches");
	if (dwt_hip_features1d_batch(DWT_HIP_FEATURE_BIT(DWT_HIP_FEATURE_WPS), d, stride_x, stride_y, rows, n, jd + 1, 2.f, dfv, count))
		dwt_util_error("device batch call: %s\n", dwt_hip_last_error());
	const int launches = dwt_hip_get_option("stat_launches") - launches0;
	size_t downloaded = 0;
	if (dwt_hip_memcpy_d2h(from_device, dfv, (size_t)rows * count * sizeof(float)))
		dwt_util_error("download: %s\n", dwt_hip_last_error());
	downloaded += (size_t)rows * count * sizeof(float);
	int bad_device = jd != j || launches != 1 || memcmp(from_device, by_row, (size_t)rows * count * sizeof(float)) != 0;
	/* the reference's per-row entry on device rows (its vector is host memory): the same numbers */
	for (int y = 0; y < rows; y += 17) {
		dwt_util_wps_s(d + (size_t)y * n, stride_x, stride_y, n, 1, n, 1, jd + 1, row_fv);
		bad_device |= memcmp(row_fv, by_row + (size_t)y * count, count * sizeof(float)) != 0;
	}
	dwt_util_log(LOG_INFO, "device rows: %d launch(es), %zu bytes downloaded (the feature matrix) of %zu bytes of coefficients\n",
		launches, downloaded, bytes);
	dwt_util_log(LOG_INFO, bad_device ? "device rows: features differ\n" : "device rows: success\n");

	dwt_hip_free(d);
	dwt_hip_free(dfv);
	free(spectra), free(coeffs), free(by_row), free(by_batch), free(from_device), free(row_fv);
	dwt_util_finish();
	return bad_host || bad_device;
}
