/*
 * san_bitplanes.c -- the block geometry and the size rule of the embedded bit-plane streams
 * (libdwt_amd/csrc/dwt_bitplane_geom.c: dwt_hip_bitplane_bands, dwt_hip_bitplane_block, dwt_hip_bitplane_words) under
 * AddressSanitizer / UndefinedBehaviorSanitizer.  Plain host C, no device, its own main:
 *
 *   gcc -std=c99 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1 \
 *       tests/san/san_bitplanes.c libdwt_amd/csrc/dwt_bitplane_geom.c libdwt_amd/csrc/dwt_sparse_geom.c -o san_bitplanes && ./san_bitplanes
 *
 * The tables are allocated at exactly the sizes the header promises, so a write past one is a report.  For every shape and
 * every pair of exponents the blocks of a band must tile the band exactly once, in raster order, and the blocks of a frame
 * must hold every sample once.  Any report aborts; prints "san_bitplanes: OK" at the end.  tests/test_bitplanes.py builds
 * and runs it.
 */
#include "../../include/libdwt_hip.h"

#include <limits.h>
#include <stdio.h>
#include <stdlib.h>

#define CHECK(c)                                                         \
	do {                                                                 \
		if (!(c)) {                                                      \
			fprintf(stderr, "san_bitplanes: CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); \
			exit(3);                                                     \
		}                                                                \
	} while (0)

static int ceil_log2(int x)
{
	int n = 0;
	while (n < 31 && (1 << n) < x)
		n++;
	return n;
}

/* the level count of the band entries */
static int levels(int sx, int sy, int j_max)
{
	const int lo = sx < sy ? sx : sy, hi = sx < sy ? sy : sx;
	if (j_max < 0)
		return ceil_log2(lo <= 1 ? hi : lo);
	return j_max < ceil_log2(hi) ? j_max : ceil_log2(hi);
}

/* every block of the table, one by one (all = 1) or the first and last two rows of blocks of every band */
static void one(int sx, int sy, int j_max, int cbx, int cby, int all)
{
	const int J = levels(sx, sy, j_max), n = 3 * J + 1;
	int *t = malloc(sizeof(int) * 5 * (n + 1)), *ref = malloc(sizeof(int) * 5 * (n + 1));
	CHECK(t && ref);
	CHECK(dwt_hip_bitplane_bands(sx, sy, j_max, cbx, cby, t) == n);
	CHECK(dwt_hip_sparse_bands(sx, sy, j_max, ref) == n);
	long long samples = 0, blocks = 0;
	for (int k = 0; k < n; k++) {
		const int *r = t + 5 * k;
		/* the rectangles are those of the sparse streams' band table */
		CHECK(r[0] == ref[5 * k] && r[1] == ref[5 * k + 1] && r[2] == ref[5 * k + 2] && r[3] == ref[5 * k + 3]);
		CHECK(r[4] == blocks);
		const long long nx = r[2] > 0 && r[3] > 0 ? ((long long)r[2] + (1 << cbx) - 1) >> cbx : 0;
		const long long ny = nx ? ((long long)r[3] + (1 << cby) - 1) >> cby : 0;
		for (long long by = 0; by < ny; by++) {
			if (!all && by >= 2 && by < ny - 2)
				by = ny - 2;
			for (long long bx = 0; bx < nx; bx++) {
				if (!all && bx >= 2 && bx < nx - 2)
					bx = nx - 2;
				int x = -7, y = -7, w = -7, h = -7;
				CHECK(dwt_hip_bitplane_block(t, n, cbx, cby, (int)(blocks + by * nx + bx), &x, &y, &w, &h) == 0);
				CHECK(x == r[0] + (bx << cbx) && y == r[1] + (by << cby));
				CHECK(w >= 1 && w <= 1 << cbx && h >= 1 && h <= 1 << cby);
				CHECK(w == (bx == nx - 1 ? r[2] - (int)(bx << cbx) : 1 << cbx) && h == (by == ny - 1 ? r[3] - (int)(by << cby) : 1 << cby));
				if (all)
					samples += (long long)w * h;
			}
		}
		if (!all)
			samples += (long long)r[2] * r[3];
		blocks += nx * ny;
	}
	CHECK(samples == (long long)sx * sy);
	CHECK(t[5 * n] == 0 && t[5 * n + 1] == 0 && t[5 * n + 2] == 0 && t[5 * n + 3] == 0 && t[5 * n + 4] == blocks);
	int x = -7, y = -7, w = -7, h = -7;
	CHECK(dwt_hip_bitplane_block(t, n, cbx, cby, (int)blocks, &x, &y, &w, &h) == -1 && dwt_hip_bitplane_block(t, n, cbx, cby, -1, &x, &y, &w, &h) == -1);
	CHECK(dwt_hip_bitplane_block(t, n, 1, cby, 0, &x, &y, &w, &h) == -1 && dwt_hip_bitplane_block(NULL, n, cbx, cby, 0, &x, &y, &w, &h) == -1);
	CHECK(dwt_hip_bitplane_block(t, n, cbx, cby, 0, NULL, &y, &w, &h) == -1);
	CHECK(x == -7 && y == -7 && w == -7 && h == -7);
	free(t);
	free(ref);
}

int main(void)
{
	/* the shapes of tests/test_hip_bitplanes.py, one sample, one row, one column, small odd ones, large ones */
	static const int shapes[][2] = {{5, 3}, {1, 37}, {37, 1}, {72, 40}, {264, 136}, {1, 1}, {1, 5000}, {5000, 1}, {2, 2}, {3, 2}, {7, 9},
		{131, 61}, {8, 1050000}, {4097, 513}, {4096, 4096}};
	static const int exps[][2] = {{2, 2}, {3, 5}, {6, 6}, {10, 2}, {2, 10}, {2, 3}, {5, 7}};
	for (unsigned i = 0; i < sizeof shapes / sizeof shapes[0]; i++)
		for (unsigned e = 0; e < sizeof exps / sizeof exps[0]; e++) {
			const int sx = shapes[i][0], sy = shapes[i][1];
			const int Jf = ceil_log2(sx > sy ? sx : sy);
			for (int j_max = -1; j_max <= Jf + 1; j_max++)
				one(sx, sy, j_max, exps[e][0], exps[e][1], (long long)sx * sy <= 1 << 17);
			one(sx, sy, 40, exps[e][0], exps[e][1], 0);
		}
	/* the largest frames an int counts: no overflow on the way */
	one(INT_MAX, 1, -1, 2, 2, 0);
	one(1, INT_MAX, 3, 2, 10, 0);
	one(46340, 46340, -1, 2, 2, 0);
	/* empty frames: bands without samples, no blocks */
	one(0, 0, -1, 6, 6, 1);
	one(0, 9, 2, 3, 5, 1);
	one(9, 0, 0, 2, 2, 1);
	/* refusals: nothing is written */
	int t[10] = {-5, -5, -5, -5, -5, -5, -5, -5, -5, -5};
	CHECK(dwt_hip_bitplane_bands(-1, 4, 0, 2, 2, t) == -1 && dwt_hip_bitplane_bands(4, -1, 0, 2, 2, t) == -1 && dwt_hip_bitplane_bands(4, 4, 0, 2, 2, NULL) == -1);
	CHECK(dwt_hip_bitplane_bands(46341, 46341, 0, 2, 2, t) == -1 && dwt_hip_bitplane_bands(INT_MAX, 2, 0, 2, 2, t) == -1);
	CHECK(dwt_hip_bitplane_bands(4, 4, 0, 1, 2, t) == -1 && dwt_hip_bitplane_bands(4, 4, 0, 2, 11, t) == -1 && dwt_hip_bitplane_bands(4, 4, 0, 7, 6, t) == -1);
	CHECK(dwt_hip_bitplane_bands(4, 4, 0, -1, 2, t) == -1 && dwt_hip_bitplane_bands(4, 4, 0, 2, 1, t) == -1);
	for (int k = 0; k < 10; k++)
		CHECK(t[k] == -5);
	CHECK(dwt_hip_bitplane_bands(4, 4, 0, 2, 2, t) == 1 && t[2] == 4 && t[3] == 4 && t[4] == 0 && t[9] == 1);
	/* the size rule */
	CHECK(dwt_hip_bitplane_words(16, 0) == 0 && dwt_hip_bitplane_words(16, 1) == 2 && dwt_hip_bitplane_words(185, 3) == 12);
	CHECK(dwt_hip_bitplane_words(64, 16) == 17 && dwt_hip_bitplane_words(65, 16) == 34 && dwt_hip_bitplane_words(4096, 32) == 33 * 64);
	CHECK(dwt_hip_bitplane_words(0, 1) == -1 && dwt_hip_bitplane_words(4097, 1) == -1 && dwt_hip_bitplane_words(64, -1) == -1 &&
	      dwt_hip_bitplane_words(64, 33) == -1 && dwt_hip_bitplane_words(INT_MIN, INT_MAX) == -1);
	printf("san_bitplanes: OK\n");
	return 0;
}
