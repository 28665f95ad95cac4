/*
 * nterm_approx.c -- the non-linear approximation of libdwt's examples/displ-vectors/vectors.c (:254-297) on two
 * displacement fields that stay on the device: CDF 9/7 forward of both, the N positions of largest joint magnitude
 * sqrtf(dx*dx + dy*dy) kept and every other coefficient of both transforms zeroed (dwt_hip_keep_largest_batch with two
 * channels), inverse of both.  For a few N the l2 norm of the residual magnitude is printed next to a host
 * restatement: the same transforms through host pointers, the magnitude map, qsort and the threshold loop as vectors.c
 * writes them.  Only the final fields cross PCIe (and one threshold and one count per N).  The fields are synthetic (a
 * rotation with a shear, seeded noise); no input file is read.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/nterm_approx.c -o nterm_approx \
 *       -Llibdwt_amd -l:libdwt_hip.so -Wl,-rpath,$PWD/libdwt_amd -lm
 *   ./nterm_approx
 */
#include "libdwt.h"
#include "libdwt_hip.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

enum { W = 512, H = 384, COUNT = W * H };
static const int stride_y = sizeof(float), stride_x = W * sizeof(float);
static const size_t image = (size_t)COUNT * sizeof(float);

static unsigned rnd(unsigned *s)
{
	*s = *s * 1664525u + 1013904223u;
	return *s >> 8;
}

static void make_fields(float *dx, float *dy)
{
	unsigned seed = 7u;
	for (int y = 0; y < H; y++)
		for (int x = 0; x < W; x++) {
			const float u = (float)x / W - 0.4f, v = (float)y / H - 0.55f, r2 = u * u + v * v;
			dx[(size_t)y * W + x] = -6.f * v / (1.f + 4.f * r2) + 1.5f * u * v + ((float)(rnd(&seed) & 0xffff) / 65536.f - 0.5f) * 0.02f;
			dy[(size_t)y * W + x] = 6.f * u / (1.f + 4.f * r2) - 2.f * u * u + ((float)(rnd(&seed) & 0xffff) / 65536.f - 0.5f) * 0.02f;
		}
}

static int cmp_desc(const void *a, const void *b)
{
	const float x = *(const float *)a, y = *(const float *)b;
	return x < y ? 1 : (x > y ? -1 : 0);
}

/* l2 norm of the magnitude of the difference of two pairs of fields */
static double residual(const float *ax, const float *ay, const float *bx, const float *by)
{
	double s = 0;
	for (int i = 0; i < COUNT; i++) {
		const double ex = (double)ax[i] - bx[i], ey = (double)ay[i] - by[i];
		s += ex * ex + ey * ey;
	}
	return sqrt(s);
}

int main(void)
{
	dwt_util_init();
	dwt_util_log(LOG_INFO, "library: %s on %s\n", dwt_util_version(), dwt_hip_device_name());
	float *in = malloc(2 * image), *host = malloc(2 * image), *out = malloc(2 * image), *array = malloc(image);
	make_fields(in, in + COUNT);
	/* dx and dy one after the other: a batch of two for the transforms (which take distinct source and destination), one
	 * group of two channels for the selection */
	float *d = dwt_hip_malloc(2 * image), *c = dwt_hip_malloc(2 * image), *r = dwt_hip_malloc(2 * image);
	if (!d || !c || !r || dwt_hip_memcpy_h2d(d, in, 2 * image))
		dwt_util_error("device setup: %s\n", dwt_hip_last_error());
	const int keeps[] = {COUNT / 1000, COUNT / 100, COUNT / 10, COUNT / 2, 0};
	int bad = 0;
	for (unsigned k = 0; k < sizeof(keeps) / sizeof(keeps[0]); k++) {
		int J = -1, N = keeps[k], kept = -1;
		float thr = -1.f;
		if (dwt_hip_transform2d_batch(DWT_HIP_CDF97_S, 0, d, c, image, 2, stride_x, W, H, &J))
			dwt_util_error("forward: %s\n", dwt_hip_last_error());
		const int k0 = dwt_hip_get_option("stat_launches");
		if (dwt_hip_keep_largest_batch(c, 0, 1, 2, image, stride_x, W, H, J, DWT_HIP_NTERM_FRAME, &N, &thr, &kept))
			dwt_util_error("keep: %s\n", dwt_hip_last_error());
		const int launches = dwt_hip_get_option("stat_launches") - k0;
		if (dwt_hip_transform2d_batch(DWT_HIP_CDF97_S, 1, c, r, image, 2, stride_x, W, H, &J) || dwt_hip_memcpy_d2h(out, r, 2 * image))
			dwt_util_error("inverse: %s\n", dwt_hip_last_error());

		/* the host restatement (vectors.c:250-297, then the inverse) */
		memcpy(host, in, 2 * image);
		float *hx = host, *hy = host + COUNT;
		int j = -1;
		dwt_cdf97_2f_s(hx, stride_x, stride_y, W, H, W, H, &j, 0, 0);
		j = -1;
		dwt_cdf97_2f_s(hy, stride_x, stride_y, W, H, W, H, &j, 0, 0);
		for (int i = 0; i < COUNT; i++)
			array[i] = sqrtf(hx[i] * hx[i] + hy[i] * hy[i]);
		qsort(array, COUNT, sizeof(float), cmp_desc);
		if (N < 1 || N > COUNT)
			N = COUNT;
		const float t = array[N - 1];
		int n = 0;
		for (int i = 0; i < COUNT; i++) {
			if (sqrtf(hx[i] * hx[i] + hy[i] * hy[i]) < t)
				hx[i] = hy[i] = 0.f;
			else
				n++;
		}
		dwt_cdf97_2i_s(hx, stride_x, stride_y, W, H, W, H, j, 0, 0);
		dwt_cdf97_2i_s(hy, stride_x, stride_y, W, H, W, H, j, 0, 0);

		const double r_dev = residual(in, in + COUNT, out, out + COUNT), r_host = residual(in, in + COUNT, hx, hy);
		dwt_util_log(LOG_INFO, "N = %6d: threshold %g (host %g), kept %d (host %d), residual %g (host %g), %d launches\n", N, thr, t, kept, n,
			r_dev, r_host, launches);
		bad |= thr != t || kept != n || launches > 5 || !(fabs(r_dev - r_host) <= 1e-4 * (r_host + 1e-3)) || j != J;
	}
	dwt_util_log(LOG_INFO, bad ? "failure\n" : "success\n");
	dwt_hip_free(d);
	dwt_hip_free(c);
	dwt_hip_free(r);
	free(in), free(host), free(out), free(array);
	dwt_util_finish();
	return bad;
}
