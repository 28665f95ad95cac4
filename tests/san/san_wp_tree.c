/*
 * san_wp_tree.c -- the host helpers of pruned wavelet packet trees (libdwt_amd/csrc/dwt_wp_tree.c: dwt_hip_wp_best_tree,
 * dwt_hip_wp_tree_leaves) under AddressSanitizer / UndefinedBehaviorSanitizer.  Plain host C, no device, its own main:
 *
 *   gcc -std=c99 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1 \
 *       tests/san/san_wp_tree.c libdwt_amd/csrc/dwt_wp_tree.c -o san_wp_tree && ./san_wp_tree
 *
 * Every output array is allocated at exactly the size the header promises (2^levels entries, DWT_HIP_WP_TREE_WORDS words),
 * so a write past it is a report.  Any report aborts; prints "san_wp_tree: OK" at the end.  tests/test_wp_basis.py builds
 * and runs it.
 */
#include "../../include/libdwt_hip.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#define CHECK(c)                                                         \
	do {                                                                 \
		if (!(c)) {                                                      \
			fprintf(stderr, "san_wp_tree: CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); \
			exit(3);                                                     \
		}                                                                \
	} while (0)

static unsigned rnd(unsigned *s)
{
	*s = *s * 1664525u + 1013904223u;
	return *s >> 8;
}

int main(void)
{
	unsigned seed = 1;
	for (int levels = 1; levels <= DWT_HIP_WP_TREE_MAX_LEVELS; levels++)
		for (int rep = 0; rep < 20; rep++) {
			const int nt = 2 << levels, max_leaves = 1 << levels;
			double *cost = malloc((size_t)nt * sizeof *cost), total;
			uint32_t *tree = malloc(DWT_HIP_WP_TREE_WORDS * sizeof *tree);
			int *level = malloc((size_t)max_leaves * sizeof(int)), *index = malloc((size_t)max_leaves * sizeof(int));
			int *start = malloc((size_t)max_leaves * sizeof(int)), *len = malloc((size_t)max_leaves * sizeof(int));
			CHECK(cost && tree && level && index && start && len);
			for (int h = 0; h < nt; h++) /* ties, and now and then a NaN */
				cost[h] = rnd(&seed) % 97 == 0 ? NAN : (double)(rnd(&seed) % 8) / (double)(1 + (rep & 1) * h);
			CHECK(dwt_hip_wp_best_tree(levels, cost, tree, &total) == 0);
			CHECK(dwt_hip_wp_best_tree(levels, cost, NULL, NULL) == 0);
			CHECK(!(tree[0] & 1u));
			/* the smallest and a few other lengths that take this depth; the tree found, the full tree, noise */
			for (int N = 1 << levels; N < (2 << levels); N += 1 + (N - (1 << levels)) * 3) {
				int n = dwt_hip_wp_tree_leaves(N, levels, tree, level, index, start, len), pos = 0;
				CHECK(n >= 1 && n <= max_leaves);
				for (int i = 0; i < n; i++) {
					CHECK(start[i] == pos && len[i] >= 1 && level[i] <= levels && index[i] < (1 << level[i]));
					pos += len[i];
				}
				CHECK(pos == N);
				CHECK(dwt_hip_wp_tree_leaves(N, levels, tree, NULL, NULL, NULL, NULL) == n);
				for (int w = 0; w < DWT_HIP_WP_TREE_WORDS; w++)
					tree[w] = rep & 2 ? 0xffffffffu : rnd(&seed) * 2654435761u;
				n = dwt_hip_wp_tree_leaves(N, levels, tree, level, index, start, len);
				CHECK(n >= 1 && n <= max_leaves && (!(rep & 2) || n == max_leaves));
			}
			free(cost), free(tree), free(level), free(index), free(start), free(len);
		}
	uint32_t tree[DWT_HIP_WP_TREE_WORDS] = {0};
	double cost[4] = {0, 1, 0, 0};
	CHECK(dwt_hip_wp_best_tree(0, cost, tree, NULL) == -1 && dwt_hip_wp_best_tree(DWT_HIP_WP_TREE_MAX_LEVELS + 1, cost, tree, NULL) == -1);
	CHECK(dwt_hip_wp_best_tree(1, NULL, tree, NULL) == -1);
	CHECK(dwt_hip_wp_tree_leaves(1, 1, tree, NULL, NULL, NULL, NULL) == -1 && dwt_hip_wp_tree_leaves(100, 7, tree, NULL, NULL, NULL, NULL) == -1);
	CHECK(dwt_hip_wp_tree_leaves(100, 0, tree, NULL, NULL, NULL, NULL) == -1 && dwt_hip_wp_tree_leaves(100, 3, NULL, NULL, NULL, NULL, NULL) == -1);
	printf("san_wp_tree: OK\n");
	return 0;
}
