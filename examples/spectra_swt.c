/*
 * spectra_swt.c -- the flow of libdwt's examples/spectra-swt on synthetic rows: every spectrum (one per row) goes
 * through 10 levels of the stationary CDF 9/7 transform, level by level with swt_cdf97_f_ex_stride_s, and the median of
 * every level's high-pass and low-pass plane (dwt_util_band_med_s) becomes one feature -- the loop of the reference's
 * example, which keeps 2 x 11 x N floats per row and throws them away.  Here the same two feature matrices also come
 * from ONE dwt_hip_swt_features1d_batch call each on rows resident in device memory: one launch, no coefficient is
 * stored, and the only download is the feature matrix.  Both must agree bit for bit.  The rows are seeded noise over a
 * few smooth lines; no input file is read.  Own code written against include/.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/spectra_swt.c -o spectra_swt \
 *       -Llibdwt_amd -l:libdwt_hip.so -Wl,-rpath,$PWD/libdwt_amd -lm
 */
#include "libdwt.h"
#include "libdwt_hip.h"
#include "swt.h"

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

	enum { rows = 48, n = 2048, levels = 10 };
	const size_t bytes = (size_t)rows * n * sizeof(float), fv_bytes = (size_t)rows * levels * sizeof(float);
	float *spectra = malloc(bytes);
	unsigned seed = 4321;
	for (int y = 0; y < rows; y++) {
		const float centre = (float)(rnd(&seed) % n), width = 20.f + (float)(rnd(&seed) % 200);
		for (int x = 0; x < n; x++) {
			const float t = ((float)x - centre) / width;
			spectra[(size_t)y * n + x] = 1.f - 0.6f * expf(-t * t) + ((float)(rnd(&seed) & 0xffff) / 65536.f - 0.5f) * 0.05f;
		}
	}

	/* the reference's loop: per row, level by level, both planes kept, then one median per plane */
	float *xL = malloc((size_t)(levels + 1) * n * sizeof(float)), *xH = malloc((size_t)(levels + 1) * n * sizeof(float));
	float *fvH = malloc(fv_bytes), *fvL = malloc(fv_bytes);
	for (int y = 0; y < rows; y++) {
		memcpy(xL, spectra + (size_t)y * n, n * sizeof(float));
		for (int l = 0; l < levels; l++)
			swt_cdf97_f_ex_stride_s(xL + (size_t)l * n, xL + (size_t)(l + 1) * n, xH + (size_t)(l + 1) * n, n, sizeof(float), l);
		for (int l = 0; l < levels; l++) {
			fvH[y * levels + l] = dwt_util_band_med_s(xH + (size_t)(l + 1) * n, 0, sizeof(float), n, 1);
			fvL[y * levels + l] = dwt_util_band_med_s(xL + (size_t)(l + 1) * n, 0, sizeof(float), n, 1);
		}
	}
	dwt_util_log(LOG_INFO, "%d rows of %d samples, %d levels: %d calls of the per-level entry, %d medians\n", rows, n, levels,
		rows * levels, 2 * rows * levels);

	/* host rows through the batch call */
	float *batchH = malloc(fv_bytes), *batchL = malloc(fv_bytes);
	const unsigned med = DWT_HIP_FEATURE_BIT(DWT_HIP_FEATURE_MED);
	if (dwt_hip_swt_features1d_batch(DWT_HIP_CDF97_S, med, spectra, n * sizeof(float), sizeof(float), rows, n, levels, 0, 2.f, batchH, levels) ||
		dwt_hip_swt_features1d_batch(DWT_HIP_CDF97_S, med, spectra, n * sizeof(float), sizeof(float), rows, n, levels, 1, 2.f, batchL, levels))
		dwt_util_error("batch call: %s\n", dwt_hip_last_error());
	const int bad_host = memcmp(fvH, batchH, fv_bytes) != 0 || memcmp(fvL, batchL, fv_bytes) != 0;
	dwt_util_log(LOG_INFO, bad_host ? "host rows: per-row and batch features differ\n" : "host rows: success\n");

	/* device-resident rows: uploaded once; one launch per feature matrix, one download each */
	float *d = dwt_hip_malloc(bytes), *dfv = dwt_hip_malloc(2 * fv_bytes);
	if (!d || !dfv || dwt_hip_memcpy_h2d(d, spectra, bytes))
		dwt_util_error("device setup: %s\n", dwt_hip_last_error());
	const int launches0 = dwt_hip_get_option("stat_launches");
	if (dwt_hip_swt_features1d_batch(DWT_HIP_CDF97_S, med, d, n * sizeof(float), sizeof(float), rows, n, levels, 0, 2.f, dfv, levels) ||
		dwt_hip_swt_features1d_batch(DWT_HIP_CDF97_S, med, d, n * sizeof(float), sizeof(float), rows, n, levels, 1, 2.f, dfv + rows * levels, levels))
		dwt_util_error("device batch call: %s\n", dwt_hip_last_error());
	const int launches = dwt_hip_get_option("stat_launches") - launches0;
	float *from_device = malloc(2 * fv_bytes);
	if (dwt_hip_memcpy_d2h(from_device, dfv, 2 * fv_bytes))
		dwt_util_error("download: %s\n", dwt_hip_last_error());
	const int bad_device = launches != 2 || memcmp(from_device, fvH, fv_bytes) != 0 || memcmp(from_device + rows * levels, fvL, fv_bytes) != 0;
	dwt_util_log(LOG_INFO, "device rows: %d launch(es), %zu bytes downloaded (the feature matrices) of %zu bytes of coefficients never stored\n",
		launches, 2 * fv_bytes, 2 * (size_t)levels * bytes);
	dwt_util_log(LOG_INFO, bad_device ? "device rows: features differ\n" : "device rows: success\n");

	dwt_hip_free(d);
	dwt_hip_free(dfv);
	free(spectra), free(xL), free(xH), free(fvH), free(fvL), free(batchH), free(batchL), free(from_device);
	dwt_util_finish();
	return bad_host || bad_device;
}
