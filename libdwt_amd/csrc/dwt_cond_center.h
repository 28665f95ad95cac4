// dwt_cond_center.h -- the centre of a row as dwt_util_get_center1_s decides it (src/libdwt.c:25806, p = 10), in the
// device arithmetic DESIGN.md s16 pins: shared by the fused kernel (k_cond_lines, terms in LDS) and the per-operation
// kernel (k_rows_center, samples in global memory) of dwt_condition.hip -- the same code, so the same order and the same
// bits.  Included inside namespace dwt { namespace {.
#pragma once

// |x|^10 as four exact-order double products, rounded to float once: no pow, the same bits on every platform
static __device__ __forceinline__ float cond_term(float x)
{
	const double a = (double)fabsf(x), a2 = a * a, a4 = a2 * a2, a8 = a4 * a4;
	return (float)(a8 * a2);
}

// The centre of a row of n samples whose terms outside [lo, hi) are +0 (zero-filled samples: s + 0 == s, so they are
// never read); term(x) gives the term of sample x, lo <= x < hi.  Every sum is a chain of float additions in index order.
// *warn: what the reference warns about -- kCondWarnNorm: the norm is zero; kCondWarnIndex: a crossing was not found.
enum { kCondWarnNorm = 1, kCondWarnIndex = 2 };
template <class Term>
static __device__ __forceinline__ int cond_center(int n, int lo, int hi, Term term, int *warn)
{
	*warn = 0;
	constexpr int U = 8; // loads of U terms are issued together; the additions stay in index order
	float S = 0.f;
	int x = lo;
	for (; x + U <= hi; x += U) {
		float t[U];
#pragma unroll
		for (int k = 0; k < U; k++)
			t[k] = term(x + k);
#pragma unroll
		for (int k = 0; k < U; k++)
			S += t[k];
	}
	for (; x < hi; x++)
		S += term(x);
	const float norm = (float)pow((double)S, (double)(1.0f / 10.0f));
	if (0.0f == norm) {
		*warn = kCondWarnNorm;
		return n / 2;
	}
	const float half = cond_term(norm) / 2;
	int lidx = -1, ridx = -1;
	bool found = false;
	float s = 0.f;
	for (x = lo; x + U <= hi && !found; x += U) {
		float t[U];
#pragma unroll
		for (int k = 0; k < U; k++)
			t[k] = term(x + k);
#pragma unroll
		for (int k = 0; k < U; k++) {
			s += t[k];
			if (!found && s > half) {
				ridx = x + k - 1;
				found = true;
			}
		}
	}
	for (; x < hi && !found; x++) {
		s += term(x);
		if (s > half) {
			ridx = x - 1;
			found = true;
		}
	}
	found = false;
	s = 0.f;
	for (x = hi - 1; x - U + 1 >= lo && !found; x -= U) {
		float t[U];
#pragma unroll
		for (int k = 0; k < U; k++)
			t[k] = term(x - k);
#pragma unroll
		for (int k = 0; k < U; k++) {
			s += t[k];
			if (!found && s > half) {
				lidx = x - k + 1;
				found = true;
			}
		}
	}
	for (; x >= lo && !found; x--) {
		s += term(x);
		if (s > half) {
			lidx = x + 1;
			found = true;
		}
	}
	// -1 is the reference's "not found": ridx = x - 1 is -1 too when sample 0 alone crosses, and is treated alike
	if (lidx == -1 || ridx == -1)
		*warn = kCondWarnIndex;
	if (lidx == -1 && ridx == -1)
		return n / 2;
	if (lidx == -1)
		lidx = ridx;
	else if (ridx == -1)
		ridx = lidx;
	return (lidx + ridx) / 2;
}
