/*
 * spectra_best_basis.c -- one adaptive wavelet packet basis for a batch of spectra, everything resident on the device: the
 * rows (one spectrum per row) are uploaded once and conditioned (dwt_hip_rows_condition); the best-basis search runs per row
 * in ONE launch (dwt_hip_wp_best1d_batch with dst == NULL: the cost of every node and the tree of every row, Shannon cost,
 * nothing stored); the cost tables -- rows x 2^(levels+1) doubles, the only download -- are summed on the host and
 * dwt_hip_wp_best_tree picks the JOINT tree, so that the node energies of all rows are comparable features; the rows are
 * transformed in it (dwt_hip_wp_tree1d_batch, tree_stride 0), its leaves are listed in rising frequency order
 * (dwt_hip_wp_tree_leaves and the Gray code), and the transform is inverted and the round-trip error against the
 * conditioned rows printed.  The rows are seeded noise over two tones, so the joint tree is deep around the tones' bands
 * and shallow elsewhere.  Own code written against include/.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/spectra_best_basis.c -o spectra_best_basis \
 *       -Llibdwt_amd -l:libdwt_hip.so -Wl,-rpath,$PWD/libdwt_amd -lm
 */
#include "libdwt.h"
#include "libdwt_hip.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

static unsigned rnd(unsigned *s) /* a small LCG: the same rows everywhere */
{
	*s = *s * 1664525u + 1013904223u;
	return *s >> 8;
}

/* the position of leaf (level, k) on the frequency axis: the inverse Gray code of its natural index, as a fraction of [0, 1) */
static double band_start(int level, int k)
{
	int f = 0;
	for (int g = k; g; g >>= 1)
		f ^= g;
	return (double)f / (double)(1 << level);
}

int main(void)
{
	dwt_util_init();
	dwt_util_log(LOG_INFO, "library: %s on %s\n", dwt_util_version(), dwt_hip_device_name());

	enum { rows = 32, n = 4096, levels = 6, table = 2 << levels, max_leaves = 1 << levels };
	const size_t bytes = (size_t)rows * n * sizeof(float), cost_bytes = (size_t)rows * table * sizeof(double);
	const double pi = 3.14159265358979323846;
	float *spectra = malloc(bytes);
	unsigned seed = 24680;
	for (int y = 0; y < rows; y++)
		for (int x = 0; x < n; x++)
			spectra[(size_t)y * n + x] = 3.f + (float)cos(pi * 0.07 * (x + 0.5)) + 0.5f * (float)cos(pi * (0.61 + 0.0005 * y) * (x + 0.5)) +
				((float)(rnd(&seed) & 0xffff) / 65536.f - 0.5f) * 0.05f;

	float *d = dwt_hip_malloc(bytes), *coef = dwt_hip_malloc(bytes);
	double *dcost = dwt_hip_malloc(cost_bytes);
	uint32_t *dtree = dwt_hip_malloc(DWT_HIP_WP_TREE_WORDS * sizeof(uint32_t));
	if (!d || !coef || !dcost || !dtree || dwt_hip_memcpy_h2d(d, spectra, bytes))
		dwt_util_error("device setup: %s\n", dwt_hip_last_error());
	if (dwt_hip_rows_condition(DWT_HIP_ROWS_MED_SHIFT | DWT_HIP_ROWS_SCALE, d, n * sizeof(float), sizeof(float), rows, n, 0, -1.f, 1.f, NULL))
		dwt_util_error("conditioning: %s\n", dwt_hip_last_error());
	float *conditioned = malloc(bytes), *back = malloc(bytes);
	double *cost = malloc(cost_bytes), joint[table];
	if (dwt_hip_memcpy_d2h(conditioned, d, bytes))
		dwt_util_error("download: %s\n", dwt_hip_last_error());

	/* the per-row search: costs only */
	const int launches0 = dwt_hip_get_option("stat_launches");
	if (dwt_hip_wp_best1d_batch(DWT_HIP_CDF97_S, DWT_HIP_WP_COST_SHANNON, 0.f, d, NULL, n * sizeof(float), sizeof(float), rows, n, levels, NULL, 0,
			NULL, dcost, table * sizeof(double)))
		dwt_util_error("search: %s\n", dwt_hip_last_error());
	const int launches = dwt_hip_get_option("stat_launches") - launches0;
	dwt_hip_sync();
	if (dwt_hip_memcpy_d2h(cost, dcost, cost_bytes))
		dwt_util_error("download: %s\n", dwt_hip_last_error());

	/* the joint tree of the summed tables */
	uint32_t tree[DWT_HIP_WP_TREE_WORDS];
	double total, root = 0, rows_total = 0;
	memset(joint, 0, sizeof joint);
	for (int y = 0; y < rows; y++) {
		for (int h = 1; h < table; h++)
			joint[h] += cost[(size_t)y * table + h];
		rows_total += cost[(size_t)y * table]; /* entry 0: the row's own best total */
	}
	root = joint[1];
	if (dwt_hip_wp_best_tree(levels, joint, tree, &total) || dwt_hip_memcpy_h2d(dtree, tree, sizeof tree))
		dwt_util_error("joint tree\n");

	/* the rows in the joint tree (d is left untouched), and back */
	if (dwt_hip_wp_tree1d_batch(DWT_HIP_CDF97_S, 0, d, coef, n * sizeof(float), sizeof(float), rows, n, levels, dtree, 0))
		dwt_util_error("transform: %s\n", dwt_hip_last_error());
	if (dwt_hip_wp_tree1d_batch(DWT_HIP_CDF97_S, 1, coef, coef, n * sizeof(float), sizeof(float), rows, n, levels, dtree, 0))
		dwt_util_error("inverse: %s\n", dwt_hip_last_error());
	dwt_hip_sync();
	if (dwt_hip_memcpy_d2h(back, coef, bytes))
		dwt_util_error("download: %s\n", dwt_hip_last_error());

	/* the leaves, by rising frequency */
	int level[max_leaves], index[max_leaves], start[max_leaves], len[max_leaves], order[max_leaves];
	const int leaves = dwt_hip_wp_tree_leaves(n, levels, tree, level, index, start, len);
	if (leaves < 1)
		dwt_util_error("leaves\n");
	int covered = 0;
	for (int i = 0; i < leaves; i++) {
		order[i] = i;
		covered += len[i];
	}
	for (int i = 1; i < leaves; i++) /* insertion sort by the band's start */
		for (int j = i; j > 0 && band_start(level[order[j]], index[order[j]]) < band_start(level[order[j - 1]], index[order[j - 1]]); j--) {
			const int t = order[j];
			order[j] = order[j - 1];
			order[j - 1] = t;
		}
	dwt_util_log(LOG_INFO, "%d rows of %d samples, %d levels: %d launch(es), %zu bytes downloaded; joint tree of %d leaves, cost %g (root %g, rows on their own %g)\n",
		rows, n, levels, launches, cost_bytes, leaves, total, root, rows_total);
	double edge = 0;
	int bands_ok = 1;
	for (int i = 0; i < leaves; i++) {
		const int l = order[i];
		if (fabs(band_start(level[l], index[l]) - edge) > 1e-12)
			bands_ok = 0; /* the bands of the leaves tile [0, 1) */
		edge += 1.0 / (double)(1 << level[l]);
		if (i < 6 || i == leaves - 1)
			dwt_util_log(LOG_INFO, "band [%.4f, %.4f) pi: level %d, natural node %2d, samples %4d .. %4d\n", band_start(level[l], index[l]), edge, level[l],
				index[l], start[l], start[l] + len[l] - 1);
	}
	float err = 0.f;
	for (size_t i = 0; i < (size_t)rows * n; i++)
		err = fmaxf(err, fabsf(back[i] - conditioned[i]));
	/* the joint tree can be no cheaper than the rows' own trees together, and no dearer than the root */
	const int bad = launches != 1 || covered != n || !bands_ok || fabs(edge - 1.0) > 1e-12 || !(total <= root) || !(rows_total <= total + 1e-9 * (fabs(total) + fabs(root))) ||
		leaves < 2 || !(err < 1e-4f);
	dwt_util_log(LOG_INFO, "round trip: max error %g\n", err);
	dwt_util_log(LOG_INFO, bad ? "best basis: failure\n" : "best basis: success\n");

	dwt_hip_free(d);
	dwt_hip_free(coef);
	dwt_hip_free(dcost);
	dwt_hip_free(dtree);
	free(spectra), free(conditioned), free(back), free(cost);
	dwt_util_finish();
	return bad;
}
