/*
 * san_lifting.c -- the scheme check and the built-in schemes of the user-defined lifting wavelets
 * (libdwt_amd/csrc/dwt_lifting_scheme.c: dwt_hip_lifting_check, dwt_hip_lifting_builtin) under AddressSanitizer /
 * UndefinedBehaviorSanitizer.  Plain host C, no device, its own main:
 *
 *   gcc -std=c99 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1 \
 *       tests/san/san_lifting.c libdwt_amd/csrc/dwt_lifting_scheme.c -o san_lifting && ./san_lifting
 *
 * Every scheme lives in a heap block of exactly sizeof(struct dwt_hip_lifting), so a read or write past it is a report.
 * Every built-in scheme must pass the check with the reach its steps add up to; every field set to values around and far
 * beyond its range (INT_MIN, INT_MAX among them) must be refused or accepted without a report, and a refused scheme must
 * leave *reach alone.  Any report aborts; prints "san_lifting: OK" at the end.  tests/test_lifting.py builds and runs it.
 */
#include "../../include/libdwt_hip.h"

#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(c)                                                         \
	do {                                                                 \
		if (!(c)) {                                                      \
			fprintf(stderr, "san_lifting: CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); \
			exit(3);                                                     \
		}                                                                \
	} while (0)

static struct dwt_hip_lifting *fresh(int id)
{
	struct dwt_hip_lifting *s = malloc(sizeof(*s));
	CHECK(s);
	memset(s, 0xA5, sizeof(*s));
	CHECK(dwt_hip_lifting_builtin(id, s) == 0);
	return s;
}

static int refused(const struct dwt_hip_lifting *s)
{
	int reach = -77;
	const int rc = dwt_hip_lifting_check(s, &reach);
	CHECK(rc == 0 ? reach >= 1 && reach <= DWT_HIP_LIFT_MAX_STEPS * DWT_HIP_LIFT_MAX_OFFSET : reach == -77);
	return rc != 0;
}

static const int kValues[] = {INT_MIN, INT_MIN + 1, -65536, -9, -8, -7, -2, -1, 0, 1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 65536, INT_MAX - 1, INT_MAX};
#define N_VALUES ((int)(sizeof(kValues) / sizeof(kValues[0])))

int main(void)
{
	static const int reach_of[] = {4, 2, 1, 2, 4, 2, 2, 3};
	CHECK(sizeof(struct dwt_hip_lifting) == 800);
	for (int id = DWT_HIP_LIFT_CDF97; id <= DWT_HIP_LIFT_D4; id++) {
		struct dwt_hip_lifting *s = fresh(id);
		int reach = -1;
		CHECK(dwt_hip_lifting_check(s, &reach) == 0 && reach == reach_of[id]);
		CHECK(dwt_hip_lifting_check(s, NULL) == 0);
		CHECK((s->type == DWT_HIP_LIFT_I32) == (id == DWT_HIP_LIFT_CDF53_INT || id == DWT_HIP_LIFT_CDF97_INT || id == DWT_HIP_LIFT_HAAR_INT));
		CHECK(s->reserved == 0);
		/* every int field through every value */
		for (int v = 0; v < N_VALUES; v++) {
			struct dwt_hip_lifting *t = fresh(id);
			const int val = kValues[v];
			t->type = val;
			if (val != DWT_HIP_LIFT_F32 && val != DWT_HIP_LIFT_I32)
				CHECK(refused(t));
			else
				(void)refused(t); /* (the other type: the fields it reads are all there) */
			t->type = s->type, t->n_steps = val;
			if (val < 1 || val > DWT_HIP_LIFT_MAX_STEPS)
				CHECK(refused(t));
			else
				(void)refused(t); /* (steps behind the scheme's own are zeros: refused, never read past the block) */
			t->n_steps = s->n_steps, t->inverse_cols_first = val;
			CHECK(refused(t) == !(val == 1 || (val == 0 && s->type == DWT_HIP_LIFT_F32)));
			t->inverse_cols_first = s->inverse_cols_first;
			for (int k = 0; k < s->n_steps; k++) {
				struct dwt_hip_lifting_step *st = &t->steps[k];
				const struct dwt_hip_lifting_step keep = *st;
				st->parity = val;
				CHECK(refused(t) == (val != 0 && val != 1));
				*st = keep, st->n_terms = val;
				if (val < 1 || val > DWT_HIP_LIFT_MAX_TERMS)
					CHECK(refused(t));
				else
					(void)refused(t);
				*st = keep, st->sign = val;
				CHECK(refused(t) == (s->type == DWT_HIP_LIFT_I32 && val != 1 && val != -1));
				*st = keep, st->shift = val;
				CHECK(refused(t) == (s->type == DWT_HIP_LIFT_I32 && (val < 0 || val > 31)));
				*st = keep, st->add = val;
				CHECK(!refused(t));
				for (int m = 0; m < keep.n_terms; m++) {
					const int odd = val >= -DWT_HIP_LIFT_MAX_OFFSET && val <= DWT_HIP_LIFT_MAX_OFFSET && (val & 1);
					*st = keep, st->terms[m].off_a = val;
					CHECK(refused(t) == !odd);
					*st = keep, st->terms[m].off_b = val;
					CHECK(refused(t) == !(odd || val == 0));
					*st = keep, st->terms[m].num = val;
					CHECK(!refused(t));
					*st = keep, st->terms[m].coef = NAN;
					CHECK(refused(t) == (s->type == DWT_HIP_LIFT_F32));
					*st = keep, st->terms[m].coef = -INFINITY;
					CHECK(refused(t) == (s->type == DWT_HIP_LIFT_F32));
				}
				*st = keep;
			}
			CHECK(!refused(t));
			free(t);
		}
		for (int p = 0; p < 2; p++) {
			struct dwt_hip_lifting *t = fresh(id);
			t->fwd_scale[p] = INFINITY;
			CHECK(refused(t) == (s->type == DWT_HIP_LIFT_F32));
			t->fwd_scale[p] = 1.0f, t->inv_scale[p] = NAN;
			CHECK(refused(t) == (s->type == DWT_HIP_LIFT_F32));
			free(t);
		}
		free(s);
	}
	/* the largest scheme: 8 steps of 4 two-tap terms at the farthest offsets */
	{
		struct dwt_hip_lifting *s = fresh(DWT_HIP_LIFT_CDF97);
		int reach = 0;
		s->n_steps = DWT_HIP_LIFT_MAX_STEPS;
		for (int k = 0; k < DWT_HIP_LIFT_MAX_STEPS; k++) {
			s->steps[k].parity = k & 1, s->steps[k].n_terms = DWT_HIP_LIFT_MAX_TERMS;
			for (int m = 0; m < DWT_HIP_LIFT_MAX_TERMS; m++)
				s->steps[k].terms[m].coef = 0.25f, s->steps[k].terms[m].off_a = -7, s->steps[k].terms[m].off_b = 7;
		}
		CHECK(dwt_hip_lifting_check(s, &reach) == 0 && reach == 56);
		free(s);
	}
	{
		struct dwt_hip_lifting *s = malloc(sizeof(*s));
		CHECK(s);
		CHECK(dwt_hip_lifting_builtin(-1, s) != 0 && dwt_hip_lifting_builtin(DWT_HIP_LIFT_D4 + 1, s) != 0 && dwt_hip_lifting_builtin(INT_MAX, s) != 0);
		CHECK(dwt_hip_lifting_builtin(DWT_HIP_LIFT_D4, NULL) != 0 && dwt_hip_lifting_check(NULL, NULL) != 0);
		free(s);
	}
	printf("san_lifting: OK\n");
	return 0;
}
