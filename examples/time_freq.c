/*
 * time_freq.c -- the flow of libdwt's examples/spectra-tf over a batch of spectra: for the short-time Fourier transform,
 * the continuous wavelet transform and the S transform, the magnitude plane, the argument plane, the phase derivative
 * and the three ridge maps of EVERY spectrum, each by one call over device memory (dwt_hip_timefreq_batch,
 * dwt_hip_phase_derivative, dwt_hip_detect_ridges; include/libdwt_hip.h).  The planes of the last spectrum are then
 * compared, bit for bit, with what the reference's own per-spectrum entries (include/gabor.h) give on host memory.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/time_freq.c -Llibdwt_amd -l:libdwt_hip.so -Wl,-rpath,$PWD/libdwt_amd -lm
 */
#define _GNU_SOURCE /* M_PI */
#include "gabor.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

#define LINES 6
#define N 700
#define BINS 32

static int run(const char *name, int kind, float sigma, float freq, const float *spectra, const float *d_spectra, float *d_planes)
{
	const size_t row = N * sizeof(float), plane = BINS * row, all = LINES * plane;
	const float limit = 2.f * (float)M_PI;
	float *d_mag = d_planes, *d_arg = d_mag + LINES * BINS * N, *d_frq = d_arg + LINES * BINS * N, *d_rdg = d_frq + LINES * BINS * N;
	static float got[6][BINS][N], want[6][BINS][N];
	dwt_hip_timefreq_bank *bank = dwt_hip_timefreq_bank_create(kind, BINS, sigma, freq);
	int rc = !bank;
	rc = rc || dwt_hip_timefreq_batch(bank, d_spectra, row, sizeof(float), LINES, N, DWT_HIP_TIMEFREQ_ABS, d_mag, plane, row);
	rc = rc || dwt_hip_timefreq_batch(bank, d_spectra, row, sizeof(float), LINES, N, DWT_HIP_TIMEFREQ_ARG, d_arg, plane, row);
	rc = rc || dwt_hip_phase_derivative(d_arg, d_frq, row, sizeof(float), N, BINS, LINES, plane, limit);
	const float *d_last[3] = {d_mag + (LINES - 1) * BINS * N, d_arg + (LINES - 1) * BINS * N, d_frq + (LINES - 1) * BINS * N};
	for (int i = 0; i < 3 && !rc; i++)
		rc = dwt_hip_memcpy_d2h(got[i], d_last[i], plane);
	for (int k = 1; k <= 3 && !rc; k++) {
		rc = dwt_hip_detect_ridges(k, k == 2 ? d_frq : d_mag, d_rdg, row, sizeof(float), N, BINS, LINES, plane, 0.f);
		rc = rc || dwt_hip_memcpy_d2h(got[2 + k], d_rdg + (LINES - 1) * BINS * N, plane);
	}
	dwt_hip_timefreq_bank_free(bank);
	if (rc) {
		fprintf(stderr, "%s: %s\n", name, dwt_hip_last_error());
		return 1;
	}
	(void)all;
	/* the reference's entries, one spectrum, host memory */
	const float *sig = spectra + (LINES - 1) * N;
	if (kind == DWT_HIP_TIMEFREQ_FT) {
		gabor_ft_s(sig, sizeof(float), N, want[0], row, sizeof(float), BINS, sigma);
		gabor_ft_arg_s(sig, sizeof(float), N, want[1], row, sizeof(float), BINS, sigma);
	} else if (kind == DWT_HIP_TIMEFREQ_WT) {
		gabor_wt_s(sig, sizeof(float), N, want[0], row, sizeof(float), BINS, sigma, freq);
		gabor_wt_arg_s(sig, sizeof(float), N, want[1], row, sizeof(float), BINS, sigma, freq);
	} else {
		gabor_st_s(sig, sizeof(float), N, want[0], row, sizeof(float), BINS);
		gabor_st_arg_s(sig, sizeof(float), N, want[1], row, sizeof(float), BINS);
	}
	phase_derivative_s(want[1], want[2], row, sizeof(float), N, BINS, limit);
	detect_ridges1_s(want[0], want[3], row, sizeof(float), N, BINS, 0.f);
	detect_ridges2_s(want[2], want[4], row, sizeof(float), N, BINS, 0.f);
	detect_ridges3_s(want[0], want[5], row, sizeof(float), N, BINS, 0.f);
	int ridge_points = 0;
	for (int y = 0; y < BINS; y++)
		for (int x = 0; x < N; x++)
			ridge_points += got[3][y][x] != 0.f;
	const int same = !memcmp(got, want, sizeof got);
	fprintf(stderr, "%s: %s (%d spectra x %d bins x %d samples; %d ridge points in the last plane)\n", name, same ? "success" : "MISMATCH", LINES,
		BINS, N, ridge_points);
	return !same;
}

int main(void)
{
	static float spectra[LINES][N];
	for (int y = 0; y < LINES; y++)
		for (int x = 0; x < N; x++) { /* a continuum, two chirps and an absorption line */
			const float t = (float)x / N;
			spectra[y][x] = 1.f + 0.3f * cosf(40.f * (y + 1) * t * t) + 0.2f * cosf(300.f * t) - 0.5f * expf(-0.02f * (x - 100 * y) * (x - 100 * y));
		}
	dwt_util_init();
	float *d_spectra = dwt_hip_malloc(sizeof spectra), *d_planes = dwt_hip_malloc(4 * LINES * BINS * N * sizeof(float));
	if (!d_spectra || !d_planes || dwt_hip_memcpy_h2d(d_spectra, spectra, sizeof spectra)) {
		fprintf(stderr, "no device memory: %s\n", dwt_hip_last_error());
		return 1;
	}
	int bad = run("FT", DWT_HIP_TIMEFREQ_FT, 40.f, 0.f, &spectra[0][0], d_spectra, d_planes);
	bad += run("WT", DWT_HIP_TIMEFREQ_WT, 1.f, 0.999f * (float)M_PI, &spectra[0][0], d_spectra, d_planes);
	bad += run("ST", DWT_HIP_TIMEFREQ_ST, 0.f, 0.f, &spectra[0][0], d_spectra, d_planes);
	dwt_hip_free(d_spectra);
	dwt_hip_free(d_planes);
	dwt_util_finish();
	return bad != 0;
}
