/*
 * spectra_packets.c -- node energies of a wavelet packet tree as features of spectra, everything resident on the device:
 * a batch of rows (one spectrum per row) is uploaded once, conditioned (median shift, range scaling:
 * dwt_hip_rows_condition), transformed by `levels` packet levels of the CDF 9/7 wavelet in ONE launch
 * (dwt_hip_wp1d_batch), and the energy of each of its 2^levels nodes (wps) is pulled in rising frequency order
 * (dwt_hip_wp_features1d_batch): the only download is the rows x 2^levels matrix.  Then the packets are inverted and the
 * round-trip error against the conditioned rows is printed.  The rows are seeded noise over a few tones whose frequency
 * rises with the row, so the strongest band of a row rises with it (to within one band: the 9/7 filters of a deep tree
 * leak into the neighbouring band).  Own code written against include/.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/spectra_packets.c -o spectra_packets \
 *       -Llibdwt_amd -l:libdwt_hip.so -Wl,-rpath,$PWD/libdwt_amd -lm
 */
#include "libdwt.h"
#include "libdwt_hip.h"

#include <math.h>
#include <stdlib.h>

static unsigned rnd(unsigned *s) /* a small LCG: the same rows everywhere */
{
	*s = *s * 1664525u + 1013904223u;
	return *s >> 8;
}

int main(void)
{
	dwt_util_init();
	dwt_util_log(LOG_INFO, "library: %s on %s\n", dwt_util_version(), dwt_hip_device_name());

	enum { rows = 32, n = 4096, levels = 5, nodes = 1 << levels };
	const size_t bytes = (size_t)rows * n * sizeof(float), fv_bytes = (size_t)rows * nodes * sizeof(float);
	const double pi = 3.14159265358979323846;
	float *spectra = malloc(bytes);
	unsigned seed = 97531;
	for (int y = 0; y < rows; y++) /* a tone in the middle of band y of `rows` equal bands of [0, pi) */
		for (int x = 0; x < n; x++)
			spectra[(size_t)y * n + x] = 3.f + (float)cos(pi * (y + 0.5) / rows * (x + 0.5)) + ((float)(rnd(&seed) & 0xffff) / 65536.f - 0.5f) * 0.1f;

	float *d = dwt_hip_malloc(bytes), *cond = dwt_hip_malloc(bytes), *dfv = dwt_hip_malloc(fv_bytes);
	if (!d || !cond || !dfv || dwt_hip_memcpy_h2d(d, spectra, bytes))
		dwt_util_error("device setup: %s\n", dwt_hip_last_error());

	/* condition in place, keep a copy of the conditioned rows for the round trip */
	if (dwt_hip_rows_condition(DWT_HIP_ROWS_MED_SHIFT | DWT_HIP_ROWS_SCALE, d, n * sizeof(float), sizeof(float), rows, n, 0, -1.f, 1.f, NULL))
		dwt_util_error("conditioning: %s\n", dwt_hip_last_error());
	float *conditioned = malloc(bytes), *back = malloc(bytes), *fv = malloc(fv_bytes);
	if (dwt_hip_memcpy_d2h(conditioned, d, bytes))
		dwt_util_error("download: %s\n", dwt_hip_last_error());

	/* packets out of place (d is left untouched), node energies in frequency order, inverse in place */
	const int launches0 = dwt_hip_get_option("stat_launches");
	if (dwt_hip_wp1d_batch(DWT_HIP_CDF97_S, 0, d, cond, n * sizeof(float), sizeof(float), rows, n, levels))
		dwt_util_error("packets: %s\n", dwt_hip_last_error());
	const int launches = dwt_hip_get_option("stat_launches") - launches0;
	if (dwt_hip_wp_features1d_batch(DWT_HIP_FEATURE_BIT(DWT_HIP_FEATURE_WPS), cond, n * sizeof(float), sizeof(float), rows, n, levels, 1, 2.f,
			dfv, nodes))
		dwt_util_error("node energies: %s\n", dwt_hip_last_error());
	if (dwt_hip_wp1d_batch(DWT_HIP_CDF97_S, 1, cond, cond, n * sizeof(float), sizeof(float), rows, n, levels))
		dwt_util_error("inverse packets: %s\n", dwt_hip_last_error());
	if (dwt_hip_memcpy_d2h(fv, dfv, fv_bytes) || dwt_hip_memcpy_d2h(back, cond, bytes))
		dwt_util_error("download: %s\n", dwt_hip_last_error());

	/* the node table and the frequency order, as a caller would label the matrix's columns */
	int start[nodes], len[nodes], perm[nodes];
	if (dwt_hip_wp_nodes(n, levels, start, len) != nodes || dwt_hip_wp_freq_order(levels, perm) != nodes)
		dwt_util_error("node table\n");
	dwt_util_log(LOG_INFO, "%d rows of %d samples, %d levels: %d nodes of %d samples, %d launch(es), %zu bytes downloaded\n", rows, n, levels, nodes,
		len[0], launches, fv_bytes);

	int peaks_ok = 1;
	for (int y = 0; y < rows; y++) {
		int best = 0;
		for (int f = 1; f < nodes; f++)
			if (fv[y * nodes + f] > fv[y * nodes + best])
				best = f;
		if (abs(best - y * nodes / rows) > 1)
			peaks_ok = 0;
		if (y % 8 == 0)
			dwt_util_log(LOG_INFO, "row %2d: strongest band %2d (natural node %2d at sample %4d), energy %g\n", y, best, perm[best], start[perm[best]],
				fv[y * nodes + best]);
	}
	float err = 0.f;
	for (size_t i = 0; i < (size_t)rows * n; i++)
		err = fmaxf(err, fabsf(back[i] - conditioned[i]));
	const int bad = launches != 1 || !peaks_ok || !(err < 1e-4f);
	dwt_util_log(LOG_INFO, "round trip: max error %g\n", err);
	dwt_util_log(LOG_INFO, bad ? "packets: failure\n" : "packets: success\n");

	dwt_hip_free(d);
	dwt_hip_free(cond);
	dwt_hip_free(dfv);
	free(spectra), free(conditioned), free(back), free(fv);
	dwt_util_finish();
	return bad;
}
