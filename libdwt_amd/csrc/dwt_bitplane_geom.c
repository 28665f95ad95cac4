/* dwt_bitplane_geom.c -- the block geometry and the size rule of the embedded bit-plane streams (include/libdwt_hip.h;
 * DESIGN.md s36): the bands of a dense Mallat frame in stream order (dwt_hip_sparse_bands), every band cut into
 * code-blocks of 2^cb_log2_x x 2^cb_log2_y samples from its first sample on, the blocks of a band in raster order.
 * Plain C, no device: tests/san/san_bitplanes.c runs this file under the sanitizers. */
#include "../../include/libdwt_hip.h"

static int exponents_ok(int cbx, int cby) { return cbx >= 2 && cbx <= 10 && cby >= 2 && cby <= 10 && cbx + cby <= 12; }

int dwt_hip_bitplane_bands(int size_x, int size_y, int j_max, int cb_log2_x, int cb_log2_y, int *table)
{
	if (!table || !exponents_ok(cb_log2_x, cb_log2_y))
		return -1;
	/* the rectangles in stream order; the fifth column is replaced by the prefix of the bands' block counts */
	const int n = dwt_hip_sparse_bands(size_x, size_y, j_max, table);
	if (n < 0)
		return -1;
	long long first = 0;
	for (int k = 0; k < n; k++) {
		int *r = table + 5 * k;
		const long long nx = ((long long)r[2] + (1ll << cb_log2_x) - 1) >> cb_log2_x, ny = ((long long)r[3] + (1ll << cb_log2_y) - 1) >> cb_log2_y;
		r[4] = (int)first;
		first += r[2] > 0 && r[3] > 0 ? nx * ny : 0; /* (at most one block per sample: below INT_MAX) */
	}
	table[5 * n + 4] = (int)first;
	return n;
}

int dwt_hip_bitplane_block(const int *table, int bands, int cb_log2_x, int cb_log2_y, int s, int *x, int *y, int *w, int *h)
{
	if (!table || bands < 1 || bands > DWT_HIP_BAND_MAX_SLOTS || !exponents_ok(cb_log2_x, cb_log2_y) || !x || !y || !w || !h || s < 0 ||
	    s >= table[5 * bands + 4])
		return -1;
	/* the last band whose first block is not behind s (bands without blocks share their successor's first) */
	int lo = 0, hi = bands - 1;
	while (lo < hi) {
		const int mid = (lo + hi + 1) >> 1;
		if (table[5 * mid + 4] <= s)
			lo = mid;
		else
			hi = mid - 1;
	}
	const int *r = table + 5 * lo;
	const int nx = (int)(((long long)r[2] + (1ll << cb_log2_x) - 1) >> cb_log2_x);
	if (nx < 1)
		return -1;
	const int ls = s - r[4], bx = ls % nx, by = ls / nx;
	const int bx0 = bx << cb_log2_x, by0 = by << cb_log2_y;
	if (by0 >= r[3])
		return -1;
	*x = r[0] + bx0, *y = r[1] + by0;
	*w = r[2] - bx0 < (1 << cb_log2_x) ? r[2] - bx0 : 1 << cb_log2_x;
	*h = r[3] - by0 < (1 << cb_log2_y) ? r[3] - by0 : 1 << cb_log2_y;
	return 0;
}

int dwt_hip_bitplane_words(int n, int p)
{
	if (n < 1 || n > 4096 || p < 0 || p > 32)
		return -1;
	return p ? (p + 1) * ((n + 63) / 64) : 0;
}
