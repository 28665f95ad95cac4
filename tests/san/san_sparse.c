/*
 * san_sparse.c -- the stream order and the tile geometry of the sparse coefficient streams
 * (libdwt_amd/csrc/dwt_sparse_geom.c: dwt_hip_sparse_order, dwt_hip_sparse_bands, dwt_hip_sparse_tile) under
 * AddressSanitizer / UndefinedBehaviorSanitizer.  Plain host C, no device, its own main:
 *
 *   gcc -std=c99 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1 \
 *       tests/san/san_sparse.c libdwt_amd/csrc/dwt_sparse_geom.c -o san_sparse && ./san_sparse
 *
 * The tables are allocated at exactly the sizes the header promises, so a write past one is a report.  For every shape
 * the bands must be the frame's subbands, coarse to fine, and the tiles must partition every band exactly once, in
 * order.  Any report aborts; prints "san_sparse: OK" at the end.  tests/test_sparse.py builds and runs it.
 */
#include "../../include/libdwt_hip.h"

#include <limits.h>
#include <stdio.h>
#include <stdlib.h>

#define CHECK(c)                                                         \
	do {                                                                 \
		if (!(c)) {                                                      \
			fprintf(stderr, "san_sparse: CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); \
			exit(3);                                                     \
		}                                                                \
	} while (0)

#define TS DWT_HIP_SPARSE_TILE_SAMPLES

static int ceil_log2(int x)
{
	int n = 0;
	while (n < 31 && (1 << n) < x)
		n++;
	return n;
}

static int band(int size, int level) { return (int)(((long long)size + ((1ll << level) - 1)) >> level); }

/* the level count of the band entries */
static int levels(int sx, int sy, int j_max)
{
	const int lo = sx < sy ? sx : sy, hi = sx < sy ? sy : sx;
	if (j_max < 0)
		return ceil_log2(lo <= 1 ? hi : lo);
	return j_max < ceil_log2(hi) ? j_max : ceil_log2(hi);
}

/* walk_tiles: every tile of the table, one by one (all = 1) or the first and last two of every band */
static void one(int sx, int sy, int j_max, int all)
{
	const int J = levels(sx, sy, j_max), n = 3 * J + 1;
	int *order = malloc(sizeof(int) * n), *t = malloc(sizeof(int) * 5 * (n + 1));
	CHECK(order && t);
	CHECK(dwt_hip_sparse_order(J, order) == n);
	CHECK(dwt_hip_sparse_bands(sx, sy, j_max, t) == n);
	/* the order: LL, then the levels J .. 1, HL, LH, HH each; every slot once */
	CHECK(order[0] == 3 * J);
	for (int k = 1; k < n; k++)
		CHECK(order[k] == 3 * (J - 1 - (k - 1) / 3) + (k - 1) % 3);
	long long samples = 0, tiles = 0;
	for (int k = 0; k < n; k++) {
		const int *r = t + 5 * k, slot = order[k];
		const int l = slot == 3 * J ? J : slot / 3 + 1, kind = slot == 3 * J ? 3 : slot % 3;
		/* LL: left, top; HL: right half, top; LH: left, bottom; HH: right, bottom */
		const int bx0 = kind == 0 || kind == 2 ? band(sx, l) : 0, bx1 = kind == 0 || kind == 2 ? band(sx, l - 1) : band(sx, l);
		const int by0 = kind == 1 || kind == 2 ? band(sy, l) : 0, by1 = kind == 1 || kind == 2 ? band(sy, l - 1) : band(sy, l);
		const long long want = kind == 3 ? (long long)band(sx, J) * band(sy, J) : (long long)(bx1 - bx0) * (by1 - by0);
		CHECK((long long)r[2] * r[3] == want);
		if (want)
			CHECK(r[0] == bx0 && r[1] == by0 && r[2] == bx1 - bx0 && r[3] == by1 - by0);
		CHECK(r[4] == tiles);
		samples += want;
		const long long nt = (want + TS - 1) / TS;
		/* the band's tiles: consecutive, TS samples each but the last, the band exactly once */
		long long next = 0;
		for (long long i = 0; i < nt; i++) {
			if (!all && i >= 2 && i < nt - 2)
				i = nt - 2, next = i * TS;
			int b, s, c;
			CHECK(dwt_hip_sparse_tile(t, n, (int)(tiles + i), &b, &s, &c) == 0);
			CHECK(b == k && s == next && c >= 1 && c <= TS && (c == TS || i == nt - 1));
			next += c;
		}
		CHECK(next == want);
		tiles += nt;
	}
	CHECK(samples == (long long)sx * sy);
	CHECK(t[5 * n] == 0 && t[5 * n + 1] == 0 && t[5 * n + 2] == 0 && t[5 * n + 3] == 0 && t[5 * n + 4] == tiles);
	int b = -7, s = -7, c = -7;
	CHECK(dwt_hip_sparse_tile(t, n, (int)tiles, &b, &s, &c) == -1 && dwt_hip_sparse_tile(t, n, -1, &b, &s, &c) == -1);
	CHECK(b == -7 && s == -7 && c == -7);
	free(order);
	free(t);
}

int main(void)
{
	/* the shapes of tests/test_hip_sparse.py, one sample, one row, one column, small odd ones, large ones */
	static const int shapes[][2] = {{5, 3}, {1, 37}, {37, 1}, {72, 40}, {264, 136}, {1, 1}, {1, 5000}, {5000, 1}, {2, 2}, {3, 2}, {7, 9},
		{131, 61}, {8, 1050000}, {4097, 513}, {8192, 8192}};
	for (unsigned i = 0; i < sizeof shapes / sizeof shapes[0]; i++) {
		const int sx = shapes[i][0], sy = shapes[i][1];
		const int Jf = ceil_log2(sx > sy ? sx : sy);
		/* j_max: the default, 0, every count up to ceil(log2) of the larger side, and beyond it */
		for (int j_max = -1; j_max <= Jf + 3; j_max++)
			one(sx, sy, j_max, (long long)sx * sy <= 1 << 21);
		one(sx, sy, 40, 0);
	}
	/* the largest frames an int counts: no overflow on the way */
	one(INT_MAX, 1, -1, 0);
	one(1, INT_MAX, 3, 0);
	one(46340, 46340, -1, 0);
	/* empty frames: bands without samples, no tiles */
	one(0, 0, -1, 1);
	one(0, 9, 2, 1);
	one(9, 0, 0, 1);
	/* refusals: nothing is written */
	int t[10] = {-5, -5, -5, -5, -5, -5, -5, -5, -5, -5};
	CHECK(dwt_hip_sparse_bands(-1, 4, 0, t) == -1 && dwt_hip_sparse_bands(4, -1, 0, t) == -1 && dwt_hip_sparse_bands(4, 4, 0, NULL) == -1);
	CHECK(dwt_hip_sparse_bands(46341, 46341, 0, t) == -1 && dwt_hip_sparse_bands(INT_MAX, 2, 0, t) == -1);
	CHECK(dwt_hip_sparse_order(-1, t) == -1 && dwt_hip_sparse_order(32, t) == -1 && dwt_hip_sparse_order(0, NULL) == -1);
	for (int k = 0; k < 10; k++)
		CHECK(t[k] == -5);
	CHECK(dwt_hip_sparse_order(0, t) == 1 && t[0] == 0 && t[1] == -5);
	printf("san_sparse: OK\n");
	return 0;
}
