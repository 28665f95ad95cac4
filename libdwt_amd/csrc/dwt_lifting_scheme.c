/*
 * dwt_lifting_scheme.c -- the host side of the user-defined lifting wavelets (include/libdwt_hip.h): the
 * check of a scheme and its reach, the built-in schemes, and the synthesis norms and quantizer step tables of a float
 * scheme.  Plain C99, no device; tests/san/san_lifting.c and san_lifting_norms.c build this file alone
 * under the sanitizers.
 */
#include "../../include/libdwt_hip.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
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

/* ---- the synthesis norms of a float scheme (host arithmetic in double) ---- */

/* One inverse level in place: x holds the level's L coefficients, its H is a 1 at index h_at (h_at < 0: all zeros); x
 * becomes the samples, twice as many.  Nothing outside [*lo, *hi] is nonzero, before and after; the caller's line keeps
 * that span farther from both ends than any tap reaches, so no tap reflects. */
static void norm_inverse_level(const struct dwt_hip_lifting *s, double *x, long h_at, long *lo, long *hi)
{
	const double f0 = (double)s->inv_scale[0], f1 = (double)s->inv_scale[1];
	for (long i = *hi; i >= *lo; i--) { /* (backwards: 2i >= i, a coefficient is read before its place is written) */
		const double v = x[i];
		x[2 * i + 1] = 0.0;
		x[2 * i] = v * f0;
	}
	for (long i = *lo; i <= *hi && i < 2 * *lo; i++) /* (coefficients the samples did not overwrite) */
		x[i] = 0.0;
	*lo = 2 * *lo, *hi = 2 * *hi + 1;
	if (h_at >= 0)
		x[2 * h_at + 1] = f1;
	for (int k = s->n_steps - 1; k >= 0; k--) {
		const struct dwt_hip_lifting_step *st = &s->steps[k];
		int reach = 0;
		for (int t = 0; t < st->n_terms; t++) {
			const int a = abs(st->terms[t].off_a), b = abs(st->terms[t].off_b);
			reach = a > reach ? a : reach;
			reach = b > reach ? b : reach;
		}
		long first = *lo - reach, last = *hi + reach;
		first += (first ^ st->parity) & 1;
		for (long i = first; i <= last; i += 2) {
			double sum = 0.0;
			for (int t = 0; t < st->n_terms; t++) {
				const struct dwt_hip_lifting_term *tm = &st->terms[t];
				double a = x[i + tm->off_a];
				if (tm->off_b != 0)
					a = a + x[i + tm->off_b];
				const double p = (double)tm->coef * a;
				sum = t == 0 ? p : sum + p;
			}
			x[i] = x[i] - sum;
		}
		*lo -= reach, *hi += reach;
	}
}

/* The square root of a finite v > 0 by Heron's iteration from above: it falls until it has reached the root to the last
 * bit or two (the norms are specified to 1e-12).  Not sqrt(): this file is also built alone, into programs that are linked
 * without libm (tests/san/san_lifting.c). */
static double norm_root(double v)
{
	double r = v > 1.0 ? v : 1.0;
	for (int k = 0; k < 1100; k++) {
		const double next = 0.5 * (r + v / r);
		if (!(next < r))
			break;
		r = next;
	}
	return r;
}

/* coefficients of L (and of H) at the level of the impulse */
static long norm_line(int reach) { return 2 * ((long)reach + 2); }

/* the L2 norm of the line that a unit L (high 0) or H (high 1) coefficient of level j turns into; x: room for
 * norm_line(reach) << j doubles */
static double synthesis_norm(const struct dwt_hip_lifting *s, int reach, int j, int high, double *x)
{
	/* level j: norm_line(reach) coefficients each of L and H, the impulse in the middle.  A level turns a margin m of zeros
	 * at either end into at least 2m - reach, so the margins reach + 2 and reach + 1 stay above reach at every level. */
	const long mid = norm_line(reach) / 2;
	long lo = mid, hi = mid;
	memset(x, 0, (size_t)(norm_line(reach) << j) * sizeof(double));
	if (!high)
		x[mid] = 1.0;
	for (int level = j; level >= 1; level--)
		norm_inverse_level(s, x, high && level == j ? mid : -1, &lo, &hi);
	double sum = 0.0;
	for (long i = lo; i <= hi; i++)
		sum += x[i] * x[i];
	return norm_root(sum);
}

static int norms_of(const struct dwt_hip_lifting *s, int levels, double *norm_l, double *norm_h)
{
	int reach = 0;
	if (dwt_hip_lifting_check(s, &reach))
		return 1;
	if (s->type != DWT_HIP_LIFT_F32)
		return refuse("lifting: an int scheme has no synthesis norms (float schemes only)");
	if (levels < 0 || levels > DWT_HIP_QUANT_MAX_LEVELS)
		return refuse("lifting: %d levels (0 .. %d)", levels, DWT_HIP_QUANT_MAX_LEVELS);
	if (levels == 0)
		return 0;
	double *x = malloc((size_t)(norm_line(reach) << levels) * sizeof(double));
	if (!x)
		return refuse("lifting: no memory for a line of %ld samples", norm_line(reach) << levels);
	for (int j = 1; j <= levels; j++) {
		norm_l[j - 1] = synthesis_norm(s, reach, j, 0, x);
		norm_h[j - 1] = synthesis_norm(s, reach, j, 1, x);
	}
	free(x);
	return 0;
}

int dwt_hip_lifting_norms(const struct dwt_hip_lifting *scheme, int levels, double *norm_l, double *norm_h)
{
	if (!norm_l || !norm_h)
		return refuse("lifting: null pointer argument");
	return norms_of(scheme, levels, norm_l, norm_h);
}

int dwt_hip_lifting_quant_steps(const struct dwt_hip_lifting *scheme, int levels, float base_step, float *steps)
{
	if (!steps)
		return refuse("lifting: null pointer argument");
	if (!(base_step > 0.f) || !isfinite(base_step))
		return refuse("lifting: base step %g (finite and > 0)", (double)base_step);
	double nl[DWT_HIP_QUANT_MAX_LEVELS + 1], nh[DWT_HIP_QUANT_MAX_LEVELS + 1];
	if (norms_of(scheme, levels, nl + 1, nh + 1))
		return 1;
	nl[0] = 1.0; /* (no level: the samples themselves) */
	for (int j = 1; j <= levels; j++) {
		steps[3 * (j - 1) + 0] = (float)((double)base_step / (nh[j] * nl[j]));
		steps[3 * (j - 1) + 1] = (float)((double)base_step / (nl[j] * nh[j]));
		steps[3 * (j - 1) + 2] = (float)((double)base_step / (nh[j] * nh[j]));
	}
	steps[3 * levels] = (float)((double)base_step / (nl[levels] * nl[levels]));
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
