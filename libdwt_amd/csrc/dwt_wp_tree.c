/* dwt_wp_tree.c -- the host helpers of pruned wavelet packet trees (include/libdwt_hip.h): the best tree
 * of a cost table and the leaves of a tree, for the binary trees of lines and the quadtrees of images.  Plain C, no device:
 * tests/san/san_wp_tree.c and tests/san/san_wp_qtree.c run this file under the sanitizers. */
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

/* ---- quadtrees of images: node (ky, kx) of level j at q = (4^j - 1)/3 + ky*2^j + kx ---- */
#define QTREE_NODES ((4 * (1 << (2 * DWT_HIP_WP_QTREE_MAX_LEVELS)) - 1) / 3) /* the nodes of levels 0 .. MAX_LEVELS */

static int qbase(int j) { return ((1 << (2 * j)) - 1) / 3; }

int dwt_hip_wp_best_qtree(int levels, const double *cost, uint32_t *tree, double *total)
{
	double best[QTREE_NODES];
	uint32_t raw[DWT_HIP_WP_QTREE_WORDS];
	if (levels < 1 || levels > DWT_HIP_WP_QTREE_MAX_LEVELS || !cost)
		return -1;
	memset(raw, 0, sizeof raw);
	for (int q = qbase(levels); q < qbase(levels + 1); q++)
		best[q] = cost[q];
	for (int j = levels - 1; j >= 0; j--)
		for (int ky = 0; ky < (1 << j); ky++)
			for (int kx = 0; kx < (1 << j); kx++) {
				const int q = qbase(j) + (ky << j) + kx;
				const int ll = qbase(j + 1) + ((2 * ky) << (j + 1)) + 2 * kx, lh = ll + (2 << j);
				const double c = ((best[ll] + best[ll + 1]) + best[lh]) + best[lh + 1];
				if (c < cost[q]) { /* a tie and a NaN keep the parent */
					best[q] = c;
					raw[q >> 5] |= 1u << (q & 31);
				} else
					best[q] = cost[q];
			}
	/* effective bits only: parents before children */
	for (int j = 1; j < levels; j++)
		for (int ky = 0; ky < (1 << j); ky++)
			for (int kx = 0; kx < (1 << j); kx++) {
				const int q = qbase(j) + (ky << j) + kx, up = qbase(j - 1) + ((ky >> 1) << (j - 1)) + (kx >> 1);
				if (!tree_bit(raw, up))
					raw[q >> 5] &= ~(1u << (q & 31));
			}
	if (tree)
		memcpy(tree, raw, sizeof raw);
	if (total)
		*total = best[0];
	return 0;
}

/* depth first, the children in the order LL, HL, LH, HH */
static int qtree_walk(const uint32_t *tree, int levels, int j, int ky, int kx, int x0, int y0, int w, int h, int count, int *level, int *oky,
	int *okx, int *ox0, int *oy0, int *ow, int *oh)
{
	if (j < levels && tree_bit(tree, qbase(j) + (ky << j) + kx)) {
		const int wl = (w + 1) >> 1, hl = (h + 1) >> 1;
		count = qtree_walk(tree, levels, j + 1, 2 * ky, 2 * kx, x0, y0, wl, hl, count, level, oky, okx, ox0, oy0, ow, oh);
		count = qtree_walk(tree, levels, j + 1, 2 * ky, 2 * kx + 1, x0 + wl, y0, w - wl, hl, count, level, oky, okx, ox0, oy0, ow, oh);
		count = qtree_walk(tree, levels, j + 1, 2 * ky + 1, 2 * kx, x0, y0 + hl, wl, h - hl, count, level, oky, okx, ox0, oy0, ow, oh);
		return qtree_walk(tree, levels, j + 1, 2 * ky + 1, 2 * kx + 1, x0 + wl, y0 + hl, w - wl, h - hl, count, level, oky, okx, ox0, oy0, ow, oh);
	}
	if (level)
		level[count] = j;
	if (oky)
		oky[count] = ky;
	if (okx)
		okx[count] = kx;
	if (ox0)
		ox0[count] = x0;
	if (oy0)
		oy0[count] = y0;
	if (ow)
		ow[count] = w;
	if (oh)
		oh[count] = h;
	return count + 1;
}

int dwt_hip_wp_qtree_leaves(int size_x, int size_y, int levels, const uint32_t *tree, int *level, int *ky, int *kx, int *x0, int *y0, int *w,
	int *h)
{
	const int smaller = size_x < size_y ? size_x : size_y;
	if (smaller < 2 || levels < 1 || levels > DWT_HIP_WP_QTREE_MAX_LEVELS || levels > floor_log2(smaller) || !tree)
		return -1;
	return qtree_walk(tree, levels, 0, 0, 0, 0, 0, size_x, size_y, 0, level, ky, kx, x0, y0, w, h); /* (the recursion is levels + 1 deep) */
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
