/*
 * spectra_custom_wavelet.c -- the flow of spectra_features.c with a wavelet the library has no kernel of its own for,
 * through the user-defined lifting entry of line batches (dwt_hip_lifting1d_batch, include/libdwt_hip.h).  A matrix of
 * synthetic spectra, one per row, stays on the device:
 *
 *   1. the rows are conditioned in place (dwt_hip_rows_condition: median shift, scaling to [0, 1]);
 *   2. Daubechies D4 (the built-in scheme DWT_HIP_LIFT_D4) of every row, all levels, ONE launch;
 *   3. the wavelet power spectrum of every row from the same planes (dwt_hip_features1d_batch -- the lines are plain 1-D
 *      Mallat lines), the only download besides the check: the feature matrix;
 *   4. the inverse, in place, and the round-trip error against the conditioned rows;
 *   5. a lossless round trip of 16-bit samples with the S transform (DWT_HIP_LIFT_HAAR_INT), compared bit for bit;
 *   6. the quantizer step table of D4 (dwt_hip_lifting_quant_steps), printed for the first levels.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/spectra_custom_wavelet.c -o spectra_custom_wavelet \
 *       -Llibdwt_amd -l:libdwt_hip.so -Wl,-rpath,$PWD/libdwt_amd -lm
 *   ./spectra_custom_wavelet
 */
#include "libdwt.h"
#include "libdwt_hip.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

enum { ROWS = 256, N = 4096 };
static const int stride_y = 4, stride_x = N * 4;
static const size_t bytes = (size_t)ROWS * N * 4;

static unsigned rnd(unsigned *s) /* a small LCG: the same rows everywhere */
{
	*s = *s * 1664525u + 1013904223u;
	return *s >> 8;
}

#define TRY(call)                                                            \
	do {                                                                     \
		if (call) {                                                          \
			fprintf(stderr, "%s: %s\n", #call, dwt_hip_last_error());        \
			return 1;                                                        \
		}                                                                    \
	} while (0)

int main(void)
{
	dwt_util_init();
	printf("library: %s on %s\n", dwt_util_version(), dwt_hip_device_name());
	float *spectra = malloc(bytes), *conditioned = malloc(bytes), *back = malloc(bytes);
	unsigned seed = 12345;
	for (int y = 0; y < ROWS; y++) {
		const float centre = (float)(rnd(&seed) % N), width = 20.f + (float)(rnd(&seed) % 200);
		for (int x = 0; x < N; x++) {
			const float t = ((float)x - centre) / width;
			spectra[(size_t)y * N + x] = 1.f - 0.6f * expf(-t * t) + ((float)(rnd(&seed) & 0xffff) / 65536.f - 0.5f) * 0.05f;
		}
	}
	float *d = dwt_hip_malloc(bytes);
	if (!d) {
		fprintf(stderr, "device setup: %s\n", dwt_hip_last_error());
		return 1;
	}

	/* 1. condition the resident rows; their copy on the host is what the round trip is compared with */
	TRY(dwt_hip_memcpy_h2d(d, spectra, bytes));
	TRY(dwt_hip_rows_condition(DWT_HIP_ROWS_MED_SHIFT | DWT_HIP_ROWS_SCALE, d, stride_x, stride_y, ROWS, N, 20, 0.f, 1.f, NULL));
	TRY(dwt_hip_memcpy_d2h(conditioned, d, bytes));

	/* 2. D4 of every row, in place */
	struct dwt_hip_lifting d4;
	int reach = 0, J = -1;
	TRY(dwt_hip_lifting_builtin(DWT_HIP_LIFT_D4, &d4));
	TRY(dwt_hip_lifting_check(&d4, &reach));
	const int launches0 = dwt_hip_get_option("stat_launches");
	TRY(dwt_hip_lifting1d_batch(&d4, 0, d, d, stride_x, stride_y, ROWS, N, &J));
	const int launches = dwt_hip_get_option("stat_launches") - launches0;
	printf("D4 (reach %d, route %s): %d rows of %d samples, %d levels, %d launch(es)\n", reach,
		dwt_hip_lifting1d_route(&d4, N) == DWT_HIP_LIFT_FUSED ? "fused" : "steps", ROWS, N, J, launches);

	/* 3. the feature matrix from the same planes */
	const int count = dwt_util_count_subbands_s(d, stride_x, stride_y, N, 1, N, 1, J + 1);
	float *fv = malloc((size_t)ROWS * count * sizeof(float)), *dfv = dwt_hip_malloc((size_t)ROWS * count * sizeof(float));
	if (!dfv) {
		fprintf(stderr, "device setup: %s\n", dwt_hip_last_error());
		return 1;
	}
	TRY(dwt_hip_features1d_batch(DWT_HIP_FEATURE_BIT(DWT_HIP_FEATURE_WPS), d, stride_x, stride_y, ROWS, N, J + 1, 2.f, dfv, count));
	TRY(dwt_hip_memcpy_d2h(fv, dfv, (size_t)ROWS * count * sizeof(float)));
	int finite = 1;
	for (size_t i = 0; i < (size_t)ROWS * count; i++)
		finite &= isfinite(fv[i]) != 0;
	printf("WPS features: %d per row, row 0:", count);
	for (int k = 0; k < count && k < 6; k++)
		printf(" %.4g", fv[k]);
	printf(" ...\n");

	/* 4. back, in place */
	TRY(dwt_hip_lifting1d_batch(&d4, 1, d, d, stride_x, stride_y, ROWS, N, &J));
	TRY(dwt_hip_memcpy_d2h(back, d, bytes));
	double err = 0;
	for (size_t i = 0; i < (size_t)ROWS * N; i++)
		err = fmax(err, fabs((double)back[i] - conditioned[i]));
	printf("D4 round trip: largest error %.3g\n", err);
	int bad = !finite || !(err < 1e-4) || J != 12;

	/* 5. the S transform on 16-bit samples: lossless */
	int *in_i = malloc(bytes), *out_i = malloc(bytes);
	for (size_t i = 0; i < (size_t)ROWS * N; i++)
		in_i[i] = (int)(rnd(&seed) & 0xffff) - 32768;
	struct dwt_hip_lifting s_int;
	int Ji = -1;
	TRY(dwt_hip_lifting_builtin(DWT_HIP_LIFT_HAAR_INT, &s_int));
	TRY(dwt_hip_memcpy_h2d(d, in_i, bytes));
	TRY(dwt_hip_lifting1d_batch(&s_int, 0, d, d, stride_x, stride_y, ROWS, N, &Ji));
	TRY(dwt_hip_lifting1d_batch(&s_int, 1, d, d, stride_x, stride_y, ROWS, N, &Ji));
	TRY(dwt_hip_memcpy_d2h(out_i, d, bytes));
	const int same = memcmp(in_i, out_i, bytes) == 0;
	printf("S transform (HAAR_INT): %d levels, lossless round trip of %d rows: %s\n", Ji, ROWS, same ? "identical" : "DIFFERENT");
	bad |= !same;

	/* 6. what the quantizer needs for D4 planes */
	float steps[3 * 3 + 1];
	double nl[3], nh[3];
	TRY(dwt_hip_lifting_norms(&d4, 3, nl, nh));
	TRY(dwt_hip_lifting_quant_steps(&d4, 3, 1.0f / 256, steps));
	for (int j = 1; j <= 3; j++)
		printf("D4 level %d: synthesis norms L %.6f H %.6f, quantizer step of HH %.6g\n", j, nl[j - 1], nh[j - 1], steps[3 * (j - 1) + 2]);

	printf(bad ? "failure\n" : "success\n");
	dwt_hip_free(d);
	dwt_hip_free(dfv);
	free(spectra), free(conditioned), free(back), free(fv), free(in_i), free(out_i);
	dwt_util_finish();
	return bad;
}
