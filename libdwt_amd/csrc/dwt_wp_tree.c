/* dwt_wp_tree.c -- the host helpers of pruned wavelet packet trees (include/libdwt_hip.h): the best tree of
 * a cost table and the leaves of a tree.  Plain C, no device: tests/san/san_wp_tree.c runs this file under the sanitizers. */
#include "../../include/libdwt_hip.h"

#include <string.h>

static int tree_bit(const uint32_t *tree, int h) { return (int)((tree[h >> 5] >> (h & 31)) & 1u); }

static int floor_log2(int x)
{
	int n = 0;
	while (n < 30 && (2 << n) <= x)
		n++;
	return n;
}

int dwt_hip_wp_best_tree(int levels, const double *cost, uint32_t *tree, double *total)
{
	/* best[h] of levels 0 .. levels-1 (the leaves' best is their cost) */
	double best[1 << DWT_HIP_WP_TREE_MAX_LEVELS];
	uint32_t raw[DWT_HIP_WP_TREE_WORDS];
	if (levels < 1 || levels > DWT_HIP_WP_TREE_MAX_LEVELS || !cost)
		return -1;
	memset(raw, 0, sizeof raw);
	for (int h = (1 << levels) - 1; h >= 1; h--) {
		const int leaf_children = 2 * h >= (1 << levels);
		const double l = leaf_children ? cost[2 * h] : best[2 * h], r = leaf_children ? cost[2 * h + 1] : best[2 * h + 1];
		const double c = l + r;
		if (c < cost[h]) { /* a tie and a NaN keep the parent */
			best[h] = c;
			raw[h >> 5] |= 1u << (h & 31);
		} else
			best[h] = cost[h];
	}
	/* effective bits only: parents before children */
	for (int h = 2; h < (1 << levels); h++)
		if (!tree_bit(raw, h >> 1))
			raw[h >> 5] &= ~(1u << (h & 31));
	if (tree)
		memcpy(tree, raw, sizeof raw);
	if (total)
		*total = best[1];
	return 0;
}

int dwt_hip_wp_tree_leaves(int N, int levels, const uint32_t *tree, int *level, int *index, int *start, int *len)
{
	/* depth first, L child first: the leaves from left to right.  The stack holds at most one pending H child per level. */
	int sj[DWT_HIP_WP_TREE_MAX_LEVELS + 1], sk[DWT_HIP_WP_TREE_MAX_LEVELS + 1], ss[DWT_HIP_WP_TREE_MAX_LEVELS + 1], sn[DWT_HIP_WP_TREE_MAX_LEVELS + 1];
	int top = 0, count = 0;
	if (N < 2 || levels < 1 || levels > DWT_HIP_WP_TREE_MAX_LEVELS || levels > floor_log2(N) || !tree)
		return -1;
	sj[0] = 0, sk[0] = 0, ss[0] = 0, sn[0] = N;
	top = 1;
	while (top > 0) {
		int j, k, s, n;
		top--;
		j = sj[top], k = sk[top], s = ss[top], n = sn[top];
		while (j < levels && tree_bit(tree, (1 << j) + k)) {
			const int nl = (n + 1) >> 1;
			sj[top] = j + 1, sk[top] = 2 * k + 1, ss[top] = s + nl, sn[top] = n - nl; /* the H child waits */
			top++;
			j++, k = 2 * k, n = nl;
		}
		if (level)
			level[count] = j;
		if (index)
			index[count] = k;
		if (start)
			start[count] = s;
		if (len)
			len[count] = n;
		count++;
	}
	return count;
}
