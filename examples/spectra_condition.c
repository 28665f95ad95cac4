/*
 * spectra_condition.c -- the whole flow of libdwt's examples/spectra-dwt on a synthetic batch that never leaves the
 * device: the spectra are uploaded once, conditioned as the reference's program conditions them (dwt_util_shift21_med_s,
 * dwt_util_center21_s with 20 iterations), transformed row-wise with dwt_cdf97_2f1_s and reduced to wavelet power
 * spectra; the only download is the feature matrix.  The same rows conditioned through host pointers must give the same
 * bits, and the conditioning of the device batch takes one launch per entry (both steps in ONE through
 * dwt_hip_rows_condition).  The rows are seeded noise over an off-centre line; no input file is read.  Own code written
 * against include/libdwt.h -- note that the conditioning entries take sizes before strides.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/spectra_condition.c -o spectra_condition \
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
	float *spectra = malloc(bytes), *host = malloc(bytes), *back = malloc(bytes);
	unsigned seed = 4321;
	for (int y = 0; y < rows; y++) {
		const float centre = (float)(n / 8 + rnd(&seed) % (3 * n / 4)), width = 10.f + (float)(rnd(&seed) % 60);
		for (int x = 0; x < n; x++) {
			const float t = ((float)x - centre) / width;
			spectra[(size_t)y * n + x] = 1.f + 0.8f * expf(-t * t) + ((float)(rnd(&seed) & 0xffff) / 65536.f - 0.5f) * 0.02f;
		}
	}

	/* host rows through the reference's two calls */
	memcpy(host, spectra, bytes);
	dwt_util_shift21_med_s(host, n, rows, stride_x, stride_y);
	dwt_util_center21_s(host, n, rows, stride_x, stride_y, 20);

	/* the device batch: uploaded once; both steps in one launch, then transform and features where it lies */
	float *d = dwt_hip_malloc(bytes);
	int *info = malloc((size_t)rows * 4 * sizeof(int));
	if (!d || dwt_hip_memcpy_h2d(d, spectra, bytes))
		dwt_util_error("device setup: %s\n", dwt_hip_last_error());
	const int launches0 = dwt_hip_get_option("stat_launches");
	if (dwt_hip_rows_condition(DWT_HIP_ROWS_MED_SHIFT | DWT_HIP_ROWS_CENTER, d, stride_x, stride_y, rows, n, 20, 0.f, 1.f, info))
		dwt_util_error("conditioning: %s\n", dwt_hip_last_error());
	const int launches = dwt_hip_get_option("stat_launches") - launches0;
	int moved = 0, off_centre = 0;
	for (int y = 0; y < rows; y++) {
		moved += info[4 * y + 1] > 0;
		off_centre += dwt_util_get_center1_s(d + (size_t)y * n, n, stride_y) != n / 2 && info[4 * y + 1] < 20;
	}
	/* (a check, not part of the flow: the conditioned batch equals the host rows bit for bit) */
	if (dwt_hip_memcpy_d2h(back, d, bytes))
		dwt_util_error("download: %s\n", dwt_hip_last_error());
	const int differ = memcmp(back, host, bytes) != 0;
	dwt_util_log(LOG_INFO, "conditioning: %d launch(es), %d of %d rows moved, %d left off centre, host and device rows %s\n", launches, moved, rows,
		off_centre, differ ? "DIFFER" : "agree");

	int j = -1;
	dwt_cdf97_2f1_s(d, stride_x, stride_y, n, rows, n, rows, &j, 0);
	const int count = dwt_util_count_subbands_s(d, stride_x, stride_y, n, 1, n, 1, j + 1);
	float *dfv = dwt_hip_malloc((size_t)rows * count * sizeof(float)), *fv = malloc((size_t)rows * count * sizeof(float));
	if (!dfv || dwt_hip_features1d_batch(DWT_HIP_FEATURE_BIT(DWT_HIP_FEATURE_WPS), d, stride_x, stride_y, rows, n, j + 1, 2.f, dfv, count) ||
		dwt_hip_memcpy_d2h(fv, dfv, (size_t)rows * count * sizeof(float)))
		dwt_util_error("features: %s\n", dwt_hip_last_error());
	int finite = 1;
	for (size_t i = 0; i < (size_t)rows * count; i++)
		finite &= isfinite(fv[i]) != 0;
	dwt_util_log(LOG_INFO, "%d rows of %d samples, %d levels: %zu bytes downloaded (the feature matrix) of %zu bytes of spectra\n", rows, n, j,
		(size_t)rows * count * sizeof(float), bytes);
	const int bad = launches != 1 || differ || off_centre || !moved || !finite;
	dwt_util_log(LOG_INFO, bad ? "failure\n" : "success\n");

	dwt_hip_free(d);
	dwt_hip_free(dfv);
	free(spectra), free(host), free(back), free(info), free(fv);
	dwt_util_finish();
	return bad;
}
