/* dwt_window_geom.c -- what a window of the inverse 2-D transform needs of a Mallat frame (include/libdwt_hip.h;
 * DESIGN.md s30): per subband the rectangle of coefficients under the window plus the halo of K samples per level.
 * Plain C, no device: tests/san/san_window.c runs this file under the sanitizers. */
#include "../../include/libdwt_hip.h"

static int ceil_log2(int x)
{
	int n = 0;
	while (n < 31 && (1 << n) < x)
		n++;
	return n;
}

static int ceil_div_pow2(int v, int j) { return (int)(((long long)v + ((1ll << j) - 1)) >> j); }

/* lifting steps of the inverse = the halo in interleaved samples; -1: the window entries do not take this wavelet */
static int halo_of(int wavelet)
{
	switch (wavelet) {
	case DWT_HIP_CDF97_S: return 4;
	case DWT_HIP_CDF53_S:
	case DWT_HIP_CDF53_I:
	case DWT_HIP_CDF53_I16: return 2;
	case DWT_HIP_INTERP53_S: return 1;
	}
	return -1;
}

/* whole-sample symmetric reflection of i into [0, N), N >= 2 */
static long long reflect(long long i, long long N)
{
	const long long period = 2 * (N - 1);
	i %= period;
	if (i < 0)
		i += period;
	return i < N ? i : period - i;
}

/* an interval of indices, first and count */
struct span {
	int lo, n;
};

/* One line of N samples: the L and H indices that the samples [a, a + n) of its inverse depend on. */
static void need(struct span want, int N, int K, struct span *L, struct span *H)
{
	if (N == 1) {
		L->lo = 0, L->n = 1;
		H->lo = 0, H->n = 0;
		return;
	}
	const long long a = want.lo, b = (long long)want.lo + want.n;
	const long long i0 = 2 * (a / 2) - K + 1, i1 = 2 * ((b - 1) / 2) + K + 1;
	long long lo, hi;
	if (i0 >= 0 && i1 <= N - 1)
		lo = i0, hi = i1;
	else if (i0 < 0 && i1 > N - 1)
		lo = 0, hi = N - 1; /* the whole line */
	else if (i0 < 0 && -i0 <= N - 1)
		lo = 0, hi = i1 > -i0 ? i1 : -i0; /* one bounce at sample 0 */
	else if (i0 >= 0 && i1 <= 2 * ((long long)N - 1))
		lo = 2 * ((long long)N - 1) - i1 < i0 ? 2 * ((long long)N - 1) - i1 : i0, hi = N - 1; /* one at sample N - 1 */
	else {
		/* a line shorter than the halo: a few samples, folded one by one */
		lo = N, hi = -1;
		for (long long i = i0; i <= i1; i++) {
			const long long f = reflect(i, N);
			lo = f < lo ? f : lo;
			hi = f > hi ? f : hi;
		}
	}
	L->lo = (int)((lo + 1) / 2), L->n = (int)(hi / 2 - (lo + 1) / 2 + 1);
	H->lo = (int)(lo / 2), H->n = hi >= 1 ? (int)((hi - 1) / 2 - lo / 2 + 1) : 0;
	if (L->n < 0)
		L->n = 0;
	if (H->n < 0)
		H->n = 0;
}

static void put(int *xywh, int slot, int x, struct span cols, int y, struct span rows)
{
	int *r = xywh + 4 * slot;
	if (cols.n <= 0 || rows.n <= 0) {
		r[0] = r[1] = r[2] = r[3] = 0;
		return;
	}
	r[0] = x + cols.lo, r[1] = y + rows.lo, r[2] = cols.n, r[3] = rows.n;
}

int dwt_hip_window_regions(int wavelet, int size_x, int size_y, int j_max, int discard, int x0, int y0, int w, int h, int *xywh)
{
	const int K = halo_of(wavelet);
	if (K < 0 || size_x < 1 || size_y < 1 || !xywh)
		return -1;
	int J = ceil_log2(size_x < size_y ? size_x : size_y);
	if (j_max >= 0 && j_max < J)
		J = j_max;
	if (discard < 0 || discard > J)
		return -1;
	const int Wr = ceil_div_pow2(size_x, discard), Hr = ceil_div_pow2(size_y, discard);
	if (x0 < 0 || y0 < 0 || w < 1 || h < 1 || x0 > Wr - w || y0 > Hr - h)
		return -1;
	struct span X = {x0, w}, Y = {y0, h};
	for (int l = 1; l <= discard; l++)
		for (int k = 0; k < 12; k++)
			xywh[12 * (l - 1) + k] = 0;
	for (int l = discard + 1; l <= J; l++) {
		const int Wl = ceil_div_pow2(size_x, l), Hl = ceil_div_pow2(size_y, l);
		struct span Lx, Hx, Ly, Hy;
		need(X, ceil_div_pow2(size_x, l - 1), K, &Lx, &Hx);
		need(Y, ceil_div_pow2(size_y, l - 1), K, &Ly, &Hy);
		put(xywh, 3 * (l - 1) + 0, Wl, Hx, 0, Ly);
		put(xywh, 3 * (l - 1) + 1, 0, Lx, Hl, Hy);
		put(xywh, 3 * (l - 1) + 2, Wl, Hx, Hl, Hy);
		X = Lx, Y = Ly;
	}
	put(xywh, 3 * J, 0, X, 0, Y);
	return 3 * J + 1;
}
