/*
 * dwt_lifting_scheme.c -- the host side of the user-defined lifting wavelets (include/libdwt_hip.h): the
 * check of a scheme and its reach, and the built-in schemes.  Plain C99, no device; tests/san/san_lifting.c builds this
 * file alone under the sanitizers.
 */
#include "../../include/libdwt_hip.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

/* the library's error text (dwt_backend_lifting.hip); absent where this file is built alone */
__attribute__((weak)) void dwt_lifting_set_error(const char *msg);

static int refuse(const char *fmt, ...)
{
	char msg[256];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(msg, sizeof(msg), fmt, ap);
	va_end(ap);
	if (dwt_lifting_set_error)
		dwt_lifting_set_error(msg);
	return 1;
}

static int odd_offset(int off) { return off >= -DWT_HIP_LIFT_MAX_OFFSET && off <= DWT_HIP_LIFT_MAX_OFFSET && (off & 1); }

int dwt_hip_lifting_check(const struct dwt_hip_lifting *s, int *reach)
{
	if (!s)
		return refuse("lifting: null scheme");
	if (s->type != DWT_HIP_LIFT_F32 && s->type != DWT_HIP_LIFT_I32)
		return refuse("lifting: unknown sample type %d", s->type);
	const int is_int = s->type == DWT_HIP_LIFT_I32;
	if (s->n_steps < 1 || s->n_steps > DWT_HIP_LIFT_MAX_STEPS)
		return refuse("lifting: %d steps (1 .. %d)", s->n_steps, DWT_HIP_LIFT_MAX_STEPS);
	if (s->inverse_cols_first != 0 && s->inverse_cols_first != 1)
		return refuse("lifting: inverse_cols_first is %d (0 or 1)", s->inverse_cols_first);
	if (is_int && !s->inverse_cols_first)
		return refuse("lifting: an int scheme must set inverse_cols_first (the exact mirror of the forward)");
	if (!is_int)
		for (int p = 0; p < 2; p++)
			if (!isfinite(s->fwd_scale[p]) || !isfinite(s->inv_scale[p]))
				return refuse("lifting: the scale factors of parity %d are not finite", p);
	int r = 0;
	for (int k = 0; k < s->n_steps; k++) {
		const struct dwt_hip_lifting_step *st = &s->steps[k];
		if (st->parity != 0 && st->parity != 1)
			return refuse("lifting: step %d has parity %d (0 or 1)", k, st->parity);
		if (st->n_terms < 1 || st->n_terms > DWT_HIP_LIFT_MAX_TERMS)
			return refuse("lifting: step %d has %d terms (1 .. %d)", k, st->n_terms, DWT_HIP_LIFT_MAX_TERMS);
		if (is_int && st->sign != 1 && st->sign != -1)
			return refuse("lifting: step %d has sign %d (+1 or -1)", k, st->sign);
		if (is_int && (st->shift < 0 || st->shift > 31))
			return refuse("lifting: step %d shifts by %d (0 .. 31)", k, st->shift);
		int far = 0;
		for (int t = 0; t < st->n_terms; t++) {
			const struct dwt_hip_lifting_term *tm = &st->terms[t];
			if (!odd_offset(tm->off_a))
				return refuse("lifting: step %d term %d: off_a is %d (odd, -%d .. %d)", k, t, tm->off_a, DWT_HIP_LIFT_MAX_OFFSET,
					DWT_HIP_LIFT_MAX_OFFSET);
			if (tm->off_b != 0 && !odd_offset(tm->off_b))
				return refuse("lifting: step %d term %d: off_b is %d (odd, -%d .. %d, or 0)", k, t, tm->off_b, DWT_HIP_LIFT_MAX_OFFSET,
					DWT_HIP_LIFT_MAX_OFFSET);
			if (!is_int && !isfinite(tm->coef))
				return refuse("lifting: step %d term %d: the coefficient is not finite", k, t);
			const int a = tm->off_a < 0 ? -tm->off_a : tm->off_a, b = tm->off_b < 0 ? -tm->off_b : tm->off_b;
			far = a > far ? a : far;
			far = b > far ? b : far;
		}
		r += far;
	}
	if (reach)
		*reach = r;
	return 0;
}

/* ---- the built-in schemes ---- */

static struct dwt_hip_lifting_step *next_step(struct dwt_hip_lifting *s, int parity)
{
	struct dwt_hip_lifting_step *st = &s->steps[s->n_steps++];
	st->parity = parity;
	st->sign = 1;
	return st;
}

/* x[i] += coef * (x[i+off_a] + x[i+off_b]) */
static void float_step(struct dwt_hip_lifting *s, int parity, float coef, int off_a, int off_b)
{
	struct dwt_hip_lifting_step *st = next_step(s, parity);
	st->n_terms = 1;
	st->terms[0].coef = coef, st->terms[0].off_a = off_a, st->terms[0].off_b = off_b;
}

/* x[i] += sign * ((num * (x[i+off_a] + x[i+off_b]) + add) >> shift) */
static void int_step(struct dwt_hip_lifting *s, int parity, int sign, int num, int add, int shift, int off_a, int off_b)
{
	struct dwt_hip_lifting_step *st = next_step(s, parity);
	st->n_terms = 1;
	st->sign = sign, st->add = add, st->shift = shift;
	st->terms[0].num = num, st->terms[0].off_a = off_a, st->terms[0].off_b = off_b;
}

static void scales(struct dwt_hip_lifting *s, float fwd_even, float fwd_odd, float inv_even, float inv_odd)
{
	s->fwd_scale[0] = fwd_even, s->fwd_scale[1] = fwd_odd;
	s->inv_scale[0] = inv_even, s->inv_scale[1] = inv_odd;
}

int dwt_hip_lifting_builtin(int id, struct dwt_hip_lifting *s)
{
	if (!s)
		return refuse("lifting: null scheme");
	memset(s, 0, sizeof(*s));
	scales(s, 1.0f, 1.0f, 1.0f, 1.0f);
	/* sqrt 2 and sqrt 3 rounded to float (sqrtf is correctly rounded) */
	const float r2 = 1.41421356237309504880f, r3 = 1.73205080756887729353f;
	switch (id) {
	case DWT_HIP_LIFT_CDF97: { /* Cdf97S of dwt_lift.h */
		const float zeta = 1.1496043988602f;
		s->type = DWT_HIP_LIFT_F32;
		float_step(s, 1, -1.58613434342059f, -1, 1);
		float_step(s, 0, -0.0529801185729f, -1, 1);
		float_step(s, 1, 0.8829110755309f, -1, 1);
		float_step(s, 0, 0.4435068520439f, -1, 1);
		scales(s, zeta, 1.0f / zeta, 1.0f / zeta, zeta);
		return 0;
	}
	case DWT_HIP_LIFT_CDF53: /* Cdf53S */
	case DWT_HIP_LIFT_INTERP53: /* Interp53S: the predict alone */
		s->type = DWT_HIP_LIFT_F32;
		float_step(s, 1, -0.5f, -1, 1);
		if (id == DWT_HIP_LIFT_CDF53)
			float_step(s, 0, 0.25f, -1, 1);
		scales(s, 1.41421356237309504880f, 0.70710678118654752440f, 0.70710678118654752440f, 1.41421356237309504880f);
		return 0;
	case DWT_HIP_LIFT_CDF53_INT: /* Cdf53I */
		s->type = DWT_HIP_LIFT_I32, s->inverse_cols_first = 1;
		int_step(s, 1, -1, 1, 0, 1, -1, 1);
		int_step(s, 0, +1, 1, 2, 2, -1, 1);
		return 0;
	case DWT_HIP_LIFT_CDF97_INT: /* Cdf97I */
		s->type = DWT_HIP_LIFT_I32, s->inverse_cols_first = 1;
		int_step(s, 1, -1, 203, -(1 << 6), 7, -1, 1);
		int_step(s, 0, +1, -217, 1 << 11, 12, -1, 1);
		int_step(s, 1, -1, -113, -(1 << 6), 7, -1, 1);
		int_step(s, 0, +1, 1817, 1 << 11, 12, -1, 1);
		return 0;
	case DWT_HIP_LIFT_HAAR:
		s->type = DWT_HIP_LIFT_F32;
		float_step(s, 1, -1.0f, -1, 0);
		float_step(s, 0, 0.5f, 1, 0);
		return 0;
	case DWT_HIP_LIFT_HAAR_INT: /* the S transform */
		s->type = DWT_HIP_LIFT_I32, s->inverse_cols_first = 1;
		int_step(s, 1, -1, 1, 0, 0, -1, 0);
		int_step(s, 0, +1, 1, 0, 1, 1, 0);
		return 0;
	case DWT_HIP_LIFT_D4: {
		s->type = DWT_HIP_LIFT_F32;
		/* alpha: the quotient in double, rounded once */
		float_step(s, 1, (float)(-1.0 / (double)r3), 1, 0);
		struct dwt_hip_lifting_step *u = next_step(s, 0);
		u->n_terms = 2;
		u->terms[0].coef = (6.0f - 3.0f * r3) / 4.0f, u->terms[0].off_a = -1;
		u->terms[1].coef = r3 / 4.0f, u->terms[1].off_a = 1;
		float_step(s, 1, -1.0f / 3.0f, -1, 0);
		scales(s, (3.0f + r3) / (3.0f * r2), (3.0f - r3) / (3.0f * r2), (3.0f * r2) / (3.0f + r3), (3.0f * r2) / (3.0f - r3));
		return 0;
	}
	}
	return refuse("lifting: unknown built-in scheme %d", id);
}
