/*
 * texture_best_basis.c -- one adaptive wavelet packet basis for a batch of texture images, everything resident on the
 * device: the images -- two textures, an oriented grating and smooth blobs, each with a little noise -- are uploaded once;
 * the best-basis search runs per image (dwt_hip_wp_best2d_batch with dst == NULL: the cost of every node of every level,
 * Shannon cost, nothing stored); the cost tables -- images x (4^(levels+1) - 1)/3 doubles, the only download -- are summed on
 * the host and dwt_hip_wp_best_qtree picks the JOINT quadtree, so that the node energies of all images are comparable
 * features; the batch is transformed in it (dwt_hip_wp_tree2d_batch, tree_stride 0), its leaves are listed
 * (dwt_hip_wp_qtree_leaves), and the transform is inverted and the largest round-trip error printed.  Own code written
 * against include/.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/texture_best_basis.c -o texture_best_basis \
 *       -Llibdwt_amd -l:libdwt_hip.so -Wl,-rpath,$PWD/libdwt_amd -lm
 */
#include "libdwt.h"
#include "libdwt_hip.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

static unsigned rnd(unsigned *s) /* a small LCG: the same images everywhere */
{
	*s = *s * 1664525u + 1013904223u;
	return *s >> 8;
}

int main(void)
{
	dwt_util_init();
	dwt_util_log(LOG_INFO, "library: %s on %s\n", dwt_util_version(), dwt_hip_device_name());

	enum { batch = 8, size = 256, levels = 4, table = 341 /* (4^(levels+1) - 1)/3 */, max_leaves = 256 /* 4^levels */ };
	const size_t plane = (size_t)size * size, bytes = batch * plane * sizeof(float), cost_bytes = (size_t)batch * table * sizeof(double);
	const double pi = 3.14159265358979323846;
	float *images = malloc(bytes), *back = malloc(bytes);
	double *cost = malloc(cost_bytes), joint[table];
	unsigned seed = 13579;
	for (int b = 0; b < batch; b++)
		for (int y = 0; y < size; y++)
			for (int x = 0; x < size; x++) {
				const double noise = ((double)(rnd(&seed) & 0xffff) / 65536. - 0.5) * 0.01;
				const double grating = 0.06 * cos(pi * (0.62 + 0.002 * b) * (x + 0.5) + pi * 0.11 * (y + 0.5));
				const double blobs = 0.08 * cos(pi * 3.0 * x / size) * cos(pi * (2.0 + 0.1 * b) * y / size);
				images[b * plane + (size_t)y * size + x] = (float)((b & 1 ? grating : blobs) + noise); /* (|c| < 1: -e log e rewards concentration) */
			}

	float *d = dwt_hip_malloc(bytes), *coef = dwt_hip_malloc(bytes);
	double *dcost = dwt_hip_malloc(cost_bytes);
	uint32_t *dtree = dwt_hip_malloc(DWT_HIP_WP_QTREE_WORDS * sizeof(uint32_t));
	if (!d || !coef || !dcost || !dtree || dwt_hip_memcpy_h2d(d, images, bytes))
		dwt_util_error("device setup: %s\n", dwt_hip_last_error());

	/* the per-image search: costs only */
	const int launches0 = dwt_hip_get_option("stat_launches");
	if (dwt_hip_wp_best2d_batch(DWT_HIP_CDF97_S, DWT_HIP_WP_COST_SHANNON, 0.f, d, NULL, plane * sizeof(float), batch, size * sizeof(float),
			sizeof(float), size, size, levels, NULL, 0, NULL, dcost, table * sizeof(double)))
		dwt_util_error("search: %s\n", dwt_hip_last_error());
	const int launches = dwt_hip_get_option("stat_launches") - launches0;
	dwt_hip_sync();
	if (dwt_hip_memcpy_d2h(cost, dcost, cost_bytes))
		dwt_util_error("download: %s\n", dwt_hip_last_error());

	/* the joint quadtree of the summed tables */
	uint32_t tree[DWT_HIP_WP_QTREE_WORDS];
	double total;
	memset(joint, 0, sizeof joint);
	for (int b = 0; b < batch; b++)
		for (int q = 0; q < table; q++)
			joint[q] += cost[(size_t)b * table + q];
	if (dwt_hip_wp_best_qtree(levels, joint, tree, &total) || dwt_hip_memcpy_h2d(dtree, tree, sizeof tree))
		dwt_util_error("joint tree\n");

	/* the batch in the joint tree (d is left untouched), and back */
	if (dwt_hip_wp_tree2d_batch(DWT_HIP_CDF97_S, 0, d, coef, plane * sizeof(float), batch, size * sizeof(float), sizeof(float), size, size, levels,
			dtree, 0))
		dwt_util_error("transform: %s\n", dwt_hip_last_error());
	if (dwt_hip_wp_tree2d_batch(DWT_HIP_CDF97_S, 1, coef, coef, plane * sizeof(float), batch, size * sizeof(float), sizeof(float), size, size, levels,
			dtree, 0))
		dwt_util_error("inverse: %s\n", dwt_hip_last_error());
	dwt_hip_sync();
	if (dwt_hip_memcpy_d2h(back, coef, bytes))
		dwt_util_error("download: %s\n", dwt_hip_last_error());

	/* the leaves */
	int level[max_leaves], ky[max_leaves], kx[max_leaves], x0[max_leaves], y0[max_leaves], w[max_leaves], h[max_leaves];
	const int leaves = dwt_hip_wp_qtree_leaves(size, size, levels, tree, level, ky, kx, x0, y0, w, h);
	if (leaves < 1)
		dwt_util_error("leaves\n");
	long covered = 0;
	int depths = 0;
	for (int i = 0; i < leaves; i++) {
		covered += (long)w[i] * h[i];
		depths |= 1 << level[i];
		if (i < 6 || i == leaves - 1)
			dwt_util_log(LOG_INFO, "leaf %3d: level %d, node (%2d, %2d), %3d x %3d samples at (%3d, %3d)\n", i, level[i], ky[i], kx[i], w[i], h[i], x0[i],
				y0[i]);
	}
	dwt_util_log(LOG_INFO, "%d images of %d x %d, %d levels: %d launches, %zu bytes downloaded; joint quadtree of %d leaves, cost %g (root %g)\n", batch,
		size, size, levels, launches, cost_bytes, leaves, total, joint[0]);
	float err = 0.f;
	for (size_t i = 0; i < batch * plane; i++)
		err = fmaxf(err, fabsf(back[i] - images[i]));
	const int bad = launches != 2 * levels + 2 || covered != (long)plane || !(total < joint[0]) || leaves < 4 || leaves == max_leaves ||
		!(depths & (depths - 1)) || !(err < 1e-5f);
	dwt_util_log(LOG_INFO, "round trip: max error %g\n", err);
	dwt_util_log(LOG_INFO, bad ? "texture best basis: failure\n" : "texture best basis: success\n");

	dwt_hip_free(d);
	dwt_hip_free(coef);
	dwt_hip_free(dcost);
	dwt_hip_free(dtree);
	free(images), free(back), free(cost);
	dwt_util_finish();
	return bad;
}
