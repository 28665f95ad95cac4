/* dwt_sparse_geom.c -- the stream order and the tile geometry of the sparse coefficient streams (include/libdwt_hip.h;
 * DESIGN.md s32): the bands of a dense Mallat frame coarse to fine, and every band cut into tiles of
 * DWT_HIP_SPARSE_TILE_SAMPLES consecutive samples of its raster order.
 * Plain C, no device: tests/san/san_sparse.c runs this file under the sanitizers. */
#include "../../include/libdwt_hip.h"

static int ceil_log2(int x)
{
	int n = 0;
	while (n < 31 && (1 << n) < x)
		n++;
	return n;
}

static int ceil_div_pow2(int v, int j) { return (int)(((long long)v + ((1ll << j) - 1)) >> j); }

/* the level rule of the band entries (dwt_hip_band_levels) */
static int levels_of(int size_x, int size_y, int j_max)
{
	const int lo = size_x < size_y ? size_x : size_y, hi = size_x < size_y ? size_y : size_x;
	if (j_max < 0)
		return ceil_log2(lo <= 1 ? hi : lo);
	return j_max < ceil_log2(hi) ? j_max : ceil_log2(hi);
}

int dwt_hip_sparse_order(int levels, int *slots)
{
	if (levels < 0 || levels > 31 || !slots)
		return -1;
	int n = 0;
	slots[n++] = 3 * levels;
	for (int j = levels; j >= 1; j--)
		for (int k = 0; k < 3; k++)
			slots[n++] = 3 * (j - 1) + k;
	return n;
}

int dwt_hip_sparse_bands(int size_x, int size_y, int j_max, int *table)
{
	if (size_x < 0 || size_y < 0 || !table || (long long)size_x * size_y > 2147483647ll)
		return -1;
	const int J = levels_of(size_x, size_y, j_max);
	int order[DWT_HIP_BAND_MAX_SLOTS];
	const int n = dwt_hip_sparse_order(J, order);
	long long first = 0;
	for (int k = 0; k < n; k++) {
		const int slot = order[k];
		int x, y, w, h;
		if (slot == 3 * J) {
			x = 0, y = 0, w = ceil_div_pow2(size_x, J), h = ceil_div_pow2(size_y, J);
		} else {
			/* the rectangles of dwt_hip_band_geometry for a dense frame */
			const int j = slot / 3 + 1, kind = slot % 3;
			const int hx = ceil_div_pow2(size_x, j - 1) / 2, hy = ceil_div_pow2(size_y, j - 1) / 2;
			const int lx = ceil_div_pow2(size_x, j), ly = ceil_div_pow2(size_y, j);
			x = kind == 1 ? 0 : lx, y = kind == 0 ? 0 : ly;
			w = kind == 1 ? lx : hx, h = kind == 0 ? ly : hy;
		}
		if (w <= 0 || h <= 0)
			w = h = 0;
		int *r = table + 5 * k;
		r[0] = x, r[1] = y, r[2] = w, r[3] = h, r[4] = (int)first;
		first += ((long long)w * h + DWT_HIP_SPARSE_TILE_SAMPLES - 1) / DWT_HIP_SPARSE_TILE_SAMPLES;
	}
	int *r = table + 5 * n;
	r[0] = r[1] = r[2] = r[3] = 0, r[4] = (int)first;
	return n;
}

int dwt_hip_sparse_tile(const int *table, int bands, int tile, int *band, int *start, int *count)
{
	if (!table || bands < 1 || bands > DWT_HIP_BAND_MAX_SLOTS || !band || !start || !count || tile < 0 || tile >= table[5 * bands + 4])
		return -1;
	/* the last band whose first tile is not behind `tile` (bands without tiles share their successor's first) */
	int lo = 0, hi = bands - 1;
	while (lo < hi) {
		const int mid = (lo + hi + 1) >> 1;
		if (table[5 * mid + 4] <= tile)
			lo = mid;
		else
			hi = mid - 1;
	}
	const long long samples = (long long)table[5 * lo + 2] * table[5 * lo + 3];
	const long long s = (long long)(tile - table[5 * lo + 4]) * DWT_HIP_SPARSE_TILE_SAMPLES;
	const long long left = samples - s;
	*band = lo, *start = (int)s, *count = (int)(left < DWT_HIP_SPARSE_TILE_SAMPLES ? left : DWT_HIP_SPARSE_TILE_SAMPLES);
	return 0;
}
