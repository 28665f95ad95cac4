/*
 * san_lifting_norms.c -- the synthesis norms and quantizer step tables of a lifting scheme
 * (libdwt_amd/csrc/dwt_lifting_scheme.c: dwt_hip_lifting_norms, dwt_hip_lifting_quant_steps) under AddressSanitizer /
 * UndefinedBehaviorSanitizer.  Plain host C, no device, its own main:
 *
 *   gcc -std=c99 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1 \
 *       tests/san/san_lifting_norms.c libdwt_amd/csrc/dwt_lifting_scheme.c -o san_lifting_norms -lm && ./san_lifting_norms
 *
 * The result arrays are heap blocks of exactly the size the entries may write, so a write past them is a report.  Every
 * float built-in at every level count, a scheme of the largest reach (8 steps that each reach 7 samples) at the largest
 * level count -- the longest line the code allocates --, and every refusal, which must leave the results alone.  Any report
 * aborts; prints "san_lifting_norms: OK" at the end.  tests/test_lifting1d.py builds and runs it.
 */
#include "../../include/libdwt_hip.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(c)                                                         \
	do {                                                                 \
		if (!(c)) {                                                      \
			fprintf(stderr, "san_lifting_norms: CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); \
			exit(3);                                                     \
		}                                                                \
	} while (0)

#define LMAX DWT_HIP_QUANT_MAX_LEVELS

/* both entries at `levels`, into blocks of exactly levels doubles and 3*levels + 1 floats */
static void run(const struct dwt_hip_lifting *s, int levels, double *last_l, double *last_h)
{
	double *nl = malloc((size_t)(levels ? levels : 1) * sizeof(double)), *nh = malloc((size_t)(levels ? levels : 1) * sizeof(double));
	float *steps = malloc((size_t)(3 * levels + 1) * sizeof(float));
	CHECK(nl && nh && steps);
	CHECK(dwt_hip_lifting_norms(s, levels, nl, nh) == 0);
	CHECK(dwt_hip_lifting_quant_steps(s, levels, 0.5f, steps) == 0);
	for (int j = 0; j < levels; j++) {
		CHECK(isfinite(nl[j]) && nl[j] > 0.0 && isfinite(nh[j]) && nh[j] > 0.0);
		CHECK(steps[3 * j] == (float)(0.5 / (nh[j] * nl[j])) && steps[3 * j + 1] == steps[3 * j] && steps[3 * j + 2] == (float)(0.5 / (nh[j] * nh[j])));
	}
	CHECK(steps[3 * levels] == (levels ? (float)(0.5 / (nl[levels - 1] * nl[levels - 1])) : 0.5f));
	if (levels && last_l)
		*last_l = nl[levels - 1], *last_h = nh[levels - 1];
	free(nl), free(nh), free(steps);
}

int main(void)
{
	struct dwt_hip_lifting *s = malloc(sizeof(*s));
	CHECK(s);
	for (int id = DWT_HIP_LIFT_CDF97; id <= DWT_HIP_LIFT_D4; id++) {
		CHECK(dwt_hip_lifting_builtin(id, s) == 0);
		if (s->type == DWT_HIP_LIFT_I32) {
			/* an int scheme is refused, and nothing is written */
			double nl = -7.0, nh = -7.0;
			float step = -7.0f;
			CHECK(dwt_hip_lifting_norms(s, 1, &nl, &nh) != 0 && nl == -7.0 && nh == -7.0);
			CHECK(dwt_hip_lifting_quant_steps(s, 0, 1.0f, &step) != 0 && step == -7.0f);
			continue;
		}
		double l = 0, h = 0;
		for (int levels = 0; levels <= LMAX; levels++)
			run(s, levels, &l, &h);
		if (id == DWT_HIP_LIFT_HAAR) /* a unit L of level j is 2^j ones, a unit H 2^(j-1) halves and as many minus halves */
			CHECK(fabs(l - 256.0) < 1e-9 && fabs(h - 128.0) < 1e-9);
	}
	/* the largest reach at the largest level count */
	CHECK(dwt_hip_lifting_builtin(DWT_HIP_LIFT_HAAR, s) == 0);
	s->n_steps = DWT_HIP_LIFT_MAX_STEPS;
	for (int k = 0; k < DWT_HIP_LIFT_MAX_STEPS; k++) {
		memset(&s->steps[k], 0, sizeof(s->steps[k]));
		s->steps[k].parity = k & 1, s->steps[k].n_terms = 1, s->steps[k].sign = 1;
		s->steps[k].terms[0].coef = 0.125f, s->steps[k].terms[0].off_a = (k & 2) ? -DWT_HIP_LIFT_MAX_OFFSET : DWT_HIP_LIFT_MAX_OFFSET;
	}
	int reach = 0;
	CHECK(dwt_hip_lifting_check(s, &reach) == 0 && reach == DWT_HIP_LIFT_MAX_STEPS * DWT_HIP_LIFT_MAX_OFFSET);
	run(s, LMAX, NULL, NULL);
	/* ... and with every term and both taps, a few levels */
	for (int k = 0; k < DWT_HIP_LIFT_MAX_STEPS; k++) {
		s->steps[k].n_terms = DWT_HIP_LIFT_MAX_TERMS;
		for (int m = 0; m < DWT_HIP_LIFT_MAX_TERMS; m++)
			s->steps[k].terms[m].coef = 0.0625f, s->steps[k].terms[m].off_a = -7, s->steps[k].terms[m].off_b = 7;
	}
	run(s, 6, NULL, NULL);
	/* refusals: nothing is written */
	{
		double nl[LMAX + 1], nh[LMAX + 1];
		float steps[3 * LMAX + 4];
		for (int k = 0; k <= LMAX; k++)
			nl[k] = nh[k] = -7.0;
		for (int k = 0; k < 3 * LMAX + 4; k++)
			steps[k] = -7.0f;
		CHECK(dwt_hip_lifting_builtin(DWT_HIP_LIFT_D4, s) == 0);
		CHECK(dwt_hip_lifting_norms(NULL, 2, nl, nh) != 0 && dwt_hip_lifting_norms(s, 2, NULL, nh) != 0 && dwt_hip_lifting_norms(s, 2, nl, NULL) != 0);
		CHECK(dwt_hip_lifting_norms(s, -1, nl, nh) != 0 && dwt_hip_lifting_norms(s, LMAX + 1, nl, nh) != 0);
		CHECK(dwt_hip_lifting_quant_steps(NULL, 2, 1.0f, steps) != 0 && dwt_hip_lifting_quant_steps(s, 2, 1.0f, NULL) != 0);
		CHECK(dwt_hip_lifting_quant_steps(s, -1, 1.0f, steps) != 0 && dwt_hip_lifting_quant_steps(s, LMAX + 1, 1.0f, steps) != 0);
		CHECK(dwt_hip_lifting_quant_steps(s, 2, 0.0f, steps) != 0 && dwt_hip_lifting_quant_steps(s, 2, -1.0f, steps) != 0);
		CHECK(dwt_hip_lifting_quant_steps(s, 2, NAN, steps) != 0 && dwt_hip_lifting_quant_steps(s, 2, INFINITY, steps) != 0);
		s->steps[0].terms[0].off_a = 2; /* a bad scheme */
		CHECK(dwt_hip_lifting_norms(s, 2, nl, nh) != 0 && dwt_hip_lifting_quant_steps(s, 2, 1.0f, steps) != 0);
		for (int k = 0; k <= LMAX; k++)
			CHECK(nl[k] == -7.0 && nh[k] == -7.0);
		for (int k = 0; k < 3 * LMAX + 4; k++)
			CHECK(steps[k] == -7.0f);
	}
	free(s);
	printf("san_lifting_norms: OK\n");
	return 0;
}
