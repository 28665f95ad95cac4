/*
 * custom_wavelet.c -- wavelets the library has no kernel of its own for, through the user-defined lifting entry
 * (dwt_hip_lifting2d_batch, include/libdwt_hip.h).  A batch of synthetic pictures stays on the device:
 *
 *   1. Daubechies D4 (the built-in scheme DWT_HIP_LIFT_D4), 4 levels forward; the detail bands of the two finest levels
 *      shrunk by soft thresholding with the existing band operators (dwt_hip_bands_apply_batch -- the planes are plain
 *      Mallat planes); inverse; PSNR against the noise-free pictures, before and after.
 *   2. A scheme written out by hand -- the 2/6 wavelet's reversible integer lifting, x[odd] -= x[even]; x[even] +=
 *      x[odd] >> 1; d[n] += (s[n-1] - s[n+1] + 2) >> 2 -- checked by dwt_hip_lifting_check, and
 *      the S transform (DWT_HIP_LIFT_HAAR_INT): lossless round trips of 16-bit samples, compared bit for bit.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/custom_wavelet.c -o custom_wavelet \
 *       -Llibdwt_amd -l:libdwt_hip.so -Wl,-rpath,$PWD/libdwt_amd -lm
 *   ./custom_wavelet
 */
#include "libdwt.h"
#include "libdwt_hip.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

enum { W = 360, H = 200, BATCH = 3, COUNT = W * H, LEVELS = 4 };
static const int stride_x = W * 4, stride_y = 4;
static const size_t frame = (size_t)COUNT * 4;

static unsigned rnd(unsigned *s)
{
	*s = *s * 1664525u + 1013904223u;
	return *s >> 8;
}

static float picture(int b, int x, int y)
{
	const float u = (float)x / W, v = (float)y / H;
	return 0.5f + 0.3f * sinf(9.f * u + 2.f * b) * cosf(7.f * v) + (u + v > 0.9f + 0.1f * b ? 0.2f : 0.f);
}

static double psnr(const float *a, const float *b, size_t n)
{
	double s = 0;
	for (size_t i = 0; i < n; i++)
		s += ((double)a[i] - b[i]) * ((double)a[i] - b[i]);
	return s > 0 ? 10 * log10((double)n / s) : INFINITY; /* peak 1 */
}

#define TRY(call)                                                            \
	do {                                                                     \
		if (call) {                                                          \
			fprintf(stderr, "%s: %s\n", #call, dwt_hip_last_error());        \
			return 1;                                                        \
		}                                                                    \
	} while (0)

static int lossless(const char *name, const struct dwt_hip_lifting *s, const int *in, int *dev, int *coef, int *out)
{
	int J = -1;
	TRY(dwt_hip_memcpy_h2d(dev, in, BATCH * frame));
	TRY(dwt_hip_lifting2d_batch(s, 0, dev, coef, frame, BATCH, stride_x, stride_y, W, H, &J));
	TRY(dwt_hip_lifting2d_batch(s, 1, coef, coef, frame, BATCH, stride_x, stride_y, W, H, &J)); /* in place */
	TRY(dwt_hip_memcpy_d2h(out, coef, BATCH * frame));
	const int same = memcmp(in, out, BATCH * frame) == 0;
	printf("%s: %d levels, lossless round trip of %d frames: %s\n", name, J, BATCH, same ? "identical" : "DIFFERENT");
	return !same;
}

int main(void)
{
	dwt_util_init();
	printf("library: %s on %s\n", dwt_util_version(), dwt_hip_device_name());
	float *clean = malloc(BATCH * frame), *noisy = malloc(BATCH * frame), *out = malloc(BATCH * frame);
	unsigned seed = 3u;
	for (int b = 0; b < BATCH; b++)
		for (int y = 0; y < H; y++)
			for (int x = 0; x < W; x++) {
				const size_t i = (size_t)b * COUNT + (size_t)y * W + x;
				clean[i] = picture(b, x, y);
				noisy[i] = clean[i] + ((float)(rnd(&seed) & 0xffff) / 65536.f - 0.5f) * 0.2f;
			}
	float *d = dwt_hip_malloc(BATCH * frame), *c = dwt_hip_malloc(BATCH * frame);
	if (!d || !c) {
		fprintf(stderr, "device setup: %s\n", dwt_hip_last_error());
		return 1;
	}

	/* 1. D4: forward, shrink, inverse */
	struct dwt_hip_lifting d4;
	int reach = 0, J = LEVELS;
	TRY(dwt_hip_lifting_builtin(DWT_HIP_LIFT_D4, &d4));
	TRY(dwt_hip_lifting_check(&d4, &reach));
	TRY(dwt_hip_memcpy_h2d(d, noisy, BATCH * frame));
	TRY(dwt_hip_lifting2d_batch(&d4, 0, d, c, frame, BATCH, stride_x, stride_y, W, H, &J));
	int ops[DWT_HIP_BAND_MAX_SLOTS] = {0};
	float params[DWT_HIP_BAND_MAX_SLOTS] = {0};
	for (int slot = 0; slot < 3 * 2; slot++) /* HL, LH, HH of levels 1 and 2 */
		ops[slot] = DWT_HIP_BAND_SOFT, params[slot] = slot < 3 ? 0.09f : 0.05f;
	TRY(dwt_hip_bands_apply_batch(c, frame, BATCH, stride_x, W, H, J, ops, params, 0));
	TRY(dwt_hip_lifting2d_batch(&d4, 1, c, d, frame, BATCH, stride_x, stride_y, W, H, &J));
	TRY(dwt_hip_memcpy_d2h(out, d, BATCH * frame));
	const double before = psnr(clean, noisy, (size_t)BATCH * COUNT), after = psnr(clean, out, (size_t)BATCH * COUNT);
	printf("D4 (reach %d, route %s), %d levels, soft threshold on levels 1 and 2: PSNR %.2f dB -> %.2f dB\n", reach,
		dwt_hip_lifting_route(&d4) == DWT_HIP_LIFT_FUSED ? "fused" : "steps", J, before, after);
	int bad = !(after > before + 1.0);

	/* 2. reversible integer schemes: the S transform, and the 2/6 wavelet written out by hand */
	int *in_i = malloc(BATCH * frame), *out_i = malloc(BATCH * frame);
	for (size_t i = 0; i < (size_t)BATCH * COUNT; i++)
		in_i[i] = (int)(rnd(&seed) & 0xffff) - 32768;
	struct dwt_hip_lifting s_int, w26;
	TRY(dwt_hip_lifting_builtin(DWT_HIP_LIFT_HAAR_INT, &s_int));
	memset(&w26, 0, sizeof(w26));
	w26.type = DWT_HIP_LIFT_I32, w26.n_steps = 3, w26.inverse_cols_first = 1;
	/* d = odd - even */
	w26.steps[0] = (struct dwt_hip_lifting_step){.parity = 1, .n_terms = 1, .sign = -1, .terms = {{.num = 1, .off_a = -1}}};
	/* s = even + (d >> 1) */
	w26.steps[1] = (struct dwt_hip_lifting_step){.parity = 0, .n_terms = 1, .sign = +1, .shift = 1, .terms = {{.num = 1, .off_a = 1}}};
	/* d += (s[-1] - s[+1] + 2) >> 2 */
	w26.steps[2] = (struct dwt_hip_lifting_step){.parity = 1, .n_terms = 2, .sign = +1, .add = 2, .shift = 2,
		.terms = {{.num = 1, .off_a = -3}, {.num = -1, .off_a = 1}}};
	TRY(dwt_hip_lifting_check(&w26, &reach));
	printf("2/6 wavelet: reach %d, route %s\n", reach, dwt_hip_lifting_route(&w26) == DWT_HIP_LIFT_FUSED ? "fused" : "steps");
	bad |= lossless("S transform (HAAR_INT)", &s_int, in_i, (int *)d, (int *)c, out_i);
	bad |= lossless("2/6 wavelet", &w26, in_i, (int *)d, (int *)c, out_i);

	printf(bad ? "failure\n" : "success\n");
	dwt_hip_free(d);
	dwt_hip_free(c);
	free(clean), free(noisy), free(out), free(in_i), free(out_i);
	dwt_util_finish();
	return bad;
}
