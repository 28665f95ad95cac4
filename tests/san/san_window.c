/*
 * san_window.c -- the geometry of the windowed inverse (libdwt_amd/csrc/dwt_window_geom.c: dwt_hip_window_regions) under
 * AddressSanitizer / UndefinedBehaviorSanitizer.  Plain host C, no device, its own main:
 *
 *   gcc -std=c99 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1 \
 *       tests/san/san_window.c libdwt_amd/csrc/dwt_window_geom.c -o san_window && ./san_window
 *
 * The table is allocated at exactly the 4 * (3 J + 1) ints the header promises, so a write past it is a report; every
 * rectangle must lie inside its band.  Any report aborts; prints "san_window: OK" at the end.  tests/test_window.py builds
 * and runs it.
 */
#include "../../include/libdwt_hip.h"

#include <limits.h>
#include <stdio.h>
#include <stdlib.h>

#define CHECK(c)                                                         \
	do {                                                                 \
		if (!(c)) {                                                      \
			fprintf(stderr, "san_window: CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); \
			exit(3);                                                     \
		}                                                                \
	} while (0)

static unsigned rnd(unsigned *s)
{
	*s = *s * 1664525u + 1013904223u;
	return *s >> 8;
}

static int ceil_log2(int x)
{
	int n = 0;
	while (n < 31 && (1 << n) < x)
		n++;
	return n;
}

static int band(int size, int level) { return (int)(((long long)size + ((1ll << level) - 1)) >> level); }

static const int kWavelets[5] = {DWT_HIP_CDF97_S, DWT_HIP_CDF53_S, DWT_HIP_INTERP53_S, DWT_HIP_CDF53_I, DWT_HIP_CDF53_I16};

/* one call on a table of exactly the promised size; every rectangle inside its band */
static void one(int wavelet, int sx, int sy, int j_max, int r, int x0, int y0, int w, int h)
{
	int J = ceil_log2(sx < sy ? sx : sy);
	if (j_max >= 0 && j_max < J)
		J = j_max;
	int *t = malloc(sizeof(int) * 4 * (3 * J + 1));
	CHECK(t);
	CHECK(dwt_hip_window_regions(wavelet, sx, sy, j_max, r, x0, y0, w, h, t) == 3 * J + 1);
	for (int l = 1; l <= J; l++)
		for (int k = 0; k < 3; k++) {
			const int *q = t + 4 * (3 * (l - 1) + k);
			if (l <= r || q[2] == 0) {
				CHECK(q[0] == 0 && q[1] == 0 && q[2] == 0 && q[3] == 0);
				continue;
			}
			/* HL: right half, top; LH: left, bottom; HH: right, bottom */
			const int bx0 = k == 1 ? 0 : band(sx, l), bx1 = k == 1 ? band(sx, l) : band(sx, l - 1);
			const int by0 = k == 0 ? 0 : band(sy, l), by1 = k == 0 ? band(sy, l) : band(sy, l - 1);
			CHECK(q[2] > 0 && q[3] > 0 && q[0] >= bx0 && q[0] + q[2] <= bx1 && q[1] >= by0 && q[1] + q[3] <= by1);
		}
	const int *q = t + 12 * J;
	CHECK(q[2] > 0 && q[3] > 0 && q[0] >= 0 && q[1] >= 0 && q[0] + q[2] <= band(sx, J) && q[1] + q[3] <= band(sy, J));
	free(t);
}

int main(void)
{
	unsigned seed = 1;
	static const int sizes[][2] = {{1, 9}, {9, 1}, {2, 7}, {7, 2}, {5, 5}, {3, 3}, {33, 17}, {131, 61}, {37, 100}, {8192, 8192}, {4097, 513}};
	for (unsigned s = 0; s < sizeof sizes / sizeof sizes[0]; s++) {
		const int sx = sizes[s][0], sy = sizes[s][1];
		const int Jf = ceil_log2(sx < sy ? sx : sy);
		for (int wi = 0; wi < 5; wi++)
			for (int j_max = -1; j_max <= Jf + 1; j_max++) {
				const int J = j_max >= 0 && j_max < Jf ? j_max : Jf;
				for (int r = 0; r <= J; r++) {
					const int bw = band(sx, r), bh = band(sy, r);
					one(kWavelets[wi], sx, sy, j_max, r, 0, 0, bw, bh);
					one(kWavelets[wi], sx, sy, j_max, r, 0, 0, 1, 1);
					one(kWavelets[wi], sx, sy, j_max, r, bw - 1, bh - 1, 1, 1);
					one(kWavelets[wi], sx, sy, j_max, r, bw - 1, 0, 1, 1);
					one(kWavelets[wi], sx, sy, j_max, r, 0, bh - 1, 1, 1);
					for (int n = 0; n < 4; n++) {
						const int x0 = (int)(rnd(&seed) % (unsigned)bw), y0 = (int)(rnd(&seed) % (unsigned)bh);
						one(kWavelets[wi], sx, sy, j_max, r, x0, y0, 1 + (int)(rnd(&seed) % (unsigned)(bw - x0)), 1 + (int)(rnd(&seed) % (unsigned)(bh - y0)));
					}
				}
			}
	}
	/* the largest sizes an int holds: no overflow on the way */
	one(DWT_HIP_CDF97_S, INT_MAX, INT_MAX, 3, 0, INT_MAX - 5, INT_MAX - 7, 5, 7);
	one(DWT_HIP_CDF53_I16, INT_MAX, 2, -1, 1, 0, 0, 1, 1);
	one(DWT_HIP_INTERP53_S, INT_MAX, INT_MAX, -1, 31, 0, 0, 1, 1);
	/* refusals: nothing is written */
	int t[4] = {-5, -5, -5, -5};
	CHECK(dwt_hip_window_regions(DWT_HIP_CDF97_H, 8, 8, 0, 0, 0, 0, 8, 8, t) == -1);
	CHECK(dwt_hip_window_regions(DWT_HIP_CDF97_I, 8, 8, 0, 0, 0, 0, 8, 8, t) == -1);
	CHECK(dwt_hip_window_regions(DWT_HIP_CDF97_D, 8, 8, 0, 0, 0, 0, 8, 8, t) == -1);
	CHECK(dwt_hip_window_regions(7, 8, 8, 0, 0, 0, 0, 8, 8, t) == -1 && dwt_hip_window_regions(-1, 8, 8, 0, 0, 0, 0, 8, 8, t) == -1);
	CHECK(dwt_hip_window_regions(DWT_HIP_CDF97_S, 0, 8, 0, 0, 0, 0, 1, 1, t) == -1 && dwt_hip_window_regions(DWT_HIP_CDF97_S, 8, -3, 0, 0, 0, 0, 1, 1, t) == -1);
	CHECK(dwt_hip_window_regions(DWT_HIP_CDF97_S, 8, 8, 0, 1, 0, 0, 1, 1, t) == -1 && dwt_hip_window_regions(DWT_HIP_CDF97_S, 8, 8, 0, -1, 0, 0, 1, 1, t) == -1);
	CHECK(dwt_hip_window_regions(DWT_HIP_CDF97_S, 8, 8, 0, 0, 0, 0, 9, 8, t) == -1 && dwt_hip_window_regions(DWT_HIP_CDF97_S, 8, 8, 0, 0, 1, 0, 8, 8, t) == -1);
	CHECK(dwt_hip_window_regions(DWT_HIP_CDF97_S, 8, 8, 0, 0, 0, 0, 0, 8, t) == -1 && dwt_hip_window_regions(DWT_HIP_CDF97_S, 8, 8, 0, 0, 0, -1, 8, 8, t) == -1);
	CHECK(dwt_hip_window_regions(DWT_HIP_CDF97_S, 8, 8, 0, 0, INT_MAX, 0, INT_MAX, 8, t) == -1);
	CHECK(dwt_hip_window_regions(DWT_HIP_CDF97_S, 8, 8, 0, 0, 0, 0, 8, 8, NULL) == -1);
	CHECK(t[0] == -5 && t[1] == -5 && t[2] == -5 && t[3] == -5);
	printf("san_window: OK\n");
	return 0;
}
