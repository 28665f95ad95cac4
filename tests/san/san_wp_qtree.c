/*
 * san_wp_qtree.c -- the host helpers of pruned packet quadtrees (libdwt_amd/csrc/dwt_wp_tree.c: dwt_hip_wp_best_qtree,
 * dwt_hip_wp_qtree_leaves) under AddressSanitizer / UndefinedBehaviorSanitizer.  Plain host C, no device, its own main:
 *
 *   gcc -std=c99 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1 \
 *       tests/san/san_wp_qtree.c libdwt_amd/csrc/dwt_wp_tree.c -o san_wp_qtree && ./san_wp_qtree
 *
 * Every array is allocated at exactly the size the header promises ((4^(levels+1) - 1)/3 costs, 4^levels leaves,
 * DWT_HIP_WP_QTREE_WORDS words), so an access past it is a report.  Any report aborts; prints "san_wp_qtree: OK" at the
 * end.  tests/test_wp_basis2d.py builds and runs it.
 */
#include "../../include/libdwt_hip.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#define CHECK(c)                                                          \
	do {                                                                  \
		if (!(c)) {                                                       \
			fprintf(stderr, "san_wp_qtree: CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); \
			exit(3);                                                      \
		}                                                                 \
	} while (0)

static unsigned rnd(unsigned *s)
{
	*s = *s * 1664525u + 1013904223u;
	return *s >> 8;
}

int main(void)
{
	unsigned seed = 1;
	for (int levels = 1; levels <= DWT_HIP_WP_QTREE_MAX_LEVELS; levels++)
		for (int rep = 0; rep < 12; rep++) {
			const int nq = ((4 << (2 * levels)) - 1) / 3, max_leaves = 1 << (2 * levels);
			double *cost = malloc((size_t)nq * sizeof *cost), total;
			uint32_t *tree = malloc(DWT_HIP_WP_QTREE_WORDS * sizeof *tree);
			int *out[7];
			CHECK(cost && tree);
			for (int i = 0; i < 7; i++)
				CHECK((out[i] = malloc((size_t)max_leaves * sizeof(int))) != NULL);
			for (int q = 0; q < nq; q++) /* ties, and now and then a NaN */
				cost[q] = rnd(&seed) % 97 == 0 ? NAN : (double)(rnd(&seed) % 8) / (double)(1 + (rep & 1) * q);
			CHECK(dwt_hip_wp_best_qtree(levels, cost, tree, &total) == 0);
			CHECK(dwt_hip_wp_best_qtree(levels, cost, NULL, NULL) == 0);
			/* the smallest and a few other sizes that take this depth; the tree found, then the full tree or noise */
			for (int W = 1 << levels; W < (2 << levels); W += 1 + (W - (1 << levels)) * 3)
				for (int H = 1 << levels; H < (2 << levels); H += 2 + (H - (1 << levels)) * 5) {
					int n = dwt_hip_wp_qtree_leaves(W, H, levels, tree, out[0], out[1], out[2], out[3], out[4], out[5], out[6]);
					long area = 0;
					CHECK(n >= 1 && n <= max_leaves);
					for (int i = 0; i < n; i++) {
						CHECK(out[0][i] <= levels && out[1][i] < (1 << out[0][i]) && out[2][i] < (1 << out[0][i]));
						CHECK(out[5][i] >= 1 && out[6][i] >= 1 && out[3][i] >= 0 && out[4][i] >= 0);
						CHECK(out[3][i] + out[5][i] <= W && out[4][i] + out[6][i] <= H);
						area += (long)out[5][i] * out[6][i];
					}
					CHECK(area == (long)W * H);
					CHECK(dwt_hip_wp_qtree_leaves(W, H, levels, tree, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == n);
					for (int w = 0; w < DWT_HIP_WP_QTREE_WORDS; w++)
						tree[w] = rep & 2 ? 0xffffffffu : rnd(&seed) * 2654435761u;
					n = dwt_hip_wp_qtree_leaves(W, H, levels, tree, out[0], out[1], out[2], out[3], out[4], out[5], out[6]);
					CHECK(n >= 1 && n <= max_leaves && (!(rep & 2) || n == max_leaves));
				}
			free(cost), free(tree);
			for (int i = 0; i < 7; i++)
				free(out[i]);
		}
	uint32_t tree[DWT_HIP_WP_QTREE_WORDS] = {0};
	double cost[5] = {1, 0, 0, 0, 0};
	CHECK(dwt_hip_wp_best_qtree(0, cost, tree, NULL) == -1 && dwt_hip_wp_best_qtree(DWT_HIP_WP_QTREE_MAX_LEVELS + 1, cost, tree, NULL) == -1);
	CHECK(dwt_hip_wp_best_qtree(1, NULL, tree, NULL) == -1);
	CHECK(dwt_hip_wp_best_qtree(1, cost, tree, NULL) == 0 && tree[0] == 1u);
	CHECK(dwt_hip_wp_qtree_leaves(1, 8, 1, tree, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == -1);
	CHECK(dwt_hip_wp_qtree_leaves(100, 7, 3, tree, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == -1);
	CHECK(dwt_hip_wp_qtree_leaves(100, 100, 0, tree, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == -1);
	CHECK(dwt_hip_wp_qtree_leaves(100, 100, 6, tree, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == -1);
	CHECK(dwt_hip_wp_qtree_leaves(100, 100, 3, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == -1);
	printf("san_wp_qtree: OK\n");
	return 0;
}
