/*
 * hdr_tonemap.c -- the luminance flow of libdwt's examples/hdr/hdr.c, and the shrinkage flow behind src/denoise.c, on a
 * batch of images that stays on the device from upload to download:
 *
 *   hdr      shift by -min, log(c + eps), edge-avoiding CDF 5/3 forward (alpha 0.8), sign * |c|^0.70 on every detail
 *            band, inverse, exp(c) - eps, shift by +min;
 *   denoise  CDF 9/7 forward, the universal threshold of every image from the median magnitude of its HH(1) band, soft
 *            thresholding of every detail band with the image's own threshold, inverse.
 *
 * Between the transforms every step is ONE launch over the whole batch (dwt_hip_map_batch, dwt_hip_bands_apply_batch);
 * only the final images cross PCIe (and, in the denoise flow, one threshold per image).  Each flow is then restated on
 * the host -- the same transforms through host pointers, the pointwise steps as plain C loops over the bands
 * dwt_util_subband_s hands out, with libm's logf / powf / expf as hdr.c writes them -- and the largest difference is
 * printed.  The luminance is synthetic (a smooth ramp, bright spots, seeded noise); no input file is read.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/hdr_tonemap.c -o hdr_tonemap \
 *       -Llibdwt_amd -l:libdwt_hip.so -Wl,-rpath,$PWD/libdwt_amd -lm
 *   ./hdr_tonemap hdr | denoise
 */
#include "libdwt.h"
#include "libdwt_hip.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

enum { BATCH = 4, W = 512, H = 384 };
static const int stride_y = sizeof(float), stride_x = W * sizeof(float);
static const size_t image = (size_t)W * H * sizeof(float);

static unsigned rnd(unsigned *s)
{
	*s = *s * 1664525u + 1013904223u;
	return *s >> 8;
}

static void make_luminance(float *img, unsigned seed, float noise)
{
	const float cx = (float)(W / 4 + rnd(&seed) % (W / 2)), cy = (float)(H / 4 + rnd(&seed) % (H / 2));
	for (int y = 0; y < H; y++)
		for (int x = 0; x < W; x++) {
			const float r2 = ((float)x - cx) * ((float)x - cx) + ((float)y - cy) * ((float)y - cy);
			img[(size_t)y * W + x] = 0.05f + 0.6f * (float)x / W * (float)y / H + 300.f * expf(-r2 / 200.f) +
				((float)(rnd(&seed) & 0xffff) / 65536.f - 0.5f) * noise;
		}
}

/* f over every coefficient of every detail band of a J-level frame, as hdr.c walks them */
static void each_detail(float *img, int J, float (*f)(float, float), float a)
{
	for (int j = 1; j <= J; j++)
		for (int band = DWT_HL; band <= DWT_HH; band++) {
			void *p;
			int sx, sy;
			dwt_util_subband_s(img, stride_x, stride_y, W, H, W, H, j, (enum dwt_subbands)band, &p, &sx, &sy);
			for (int y = 0; y < sy; y++)
				for (int x = 0; x < sx; x++) {
					float *c = (float *)((char *)p + (size_t)y * stride_x) + x;
					*c = f(*c, a);
				}
		}
}

static float compress(float c, float beta) { return (c > 0 ? +1.f : -1.f) * powf(fabsf(c), beta); }
static float soft(float c, float t) { return c > t ? c - t : (c < -t ? c + t : 0.f); }

static void fill_detail(int *ops, float *params, int J, int op, float a)
{
	for (int k = 0; k < 3 * J; k++) {
		ops[k] = op;
		params[k] = a;
	}
	ops[3 * J] = DWT_HIP_BAND_KEEP;
	params[3 * J] = 0.f;
}

int main(int argc, char *argv[])
{
	const int denoise = argc > 1 && !strcmp(argv[1], "denoise");
	dwt_util_init();
	dwt_util_log(LOG_INFO, "library: %s on %s, flow: %s\n", dwt_util_version(), dwt_hip_device_name(), denoise ? "denoise" : "hdr");

	float *in = malloc(BATCH * image), *host = malloc(BATCH * image), *out = malloc(BATCH * image);
	for (int b = 0; b < BATCH; b++)
		make_luminance(in + (size_t)b * W * H, 100u + b, denoise ? 0.2f * (1 + b) : 0.01f);
	float *d = dwt_hip_malloc(BATCH * image);
	if (!d || dwt_hip_memcpy_h2d(d, in, BATCH * image))
		dwt_util_error("device setup: %s\n", dwt_hip_last_error());
	memcpy(host, in, BATCH * image);

	int ops[DWT_HIP_BAND_MAX_SLOTS], bad = 0, J = -1;
	float params[DWT_HIP_BAND_MAX_SLOTS];
	const int launches0 = dwt_hip_get_option("stat_launches");
	int shaping = 0; /* launches of the steps between the transforms */
	if (!denoise) {
		const float eps = 1e-5f, alpha = 0.8f, beta = 0.70f;
		float low = in[0], high;
		for (int b = 0; b < BATCH; b++) {
			float lo;
			dwt_util_find_min_max_s(in + (size_t)b * W * H, W, H, stride_x, stride_y, &lo, &high);
			low = lo < low ? lo : low;
		}
		const long wfloats = dwt_hip_eaw53_weights_layout(DWT_HIP_EAW_MALLAT, W, H, W, H, dwt_hip_band_levels(W, H, -1), NULL, NULL);
		float *dw = dwt_hip_malloc((size_t)BATCH * wfloats * sizeof(float)), *hw = malloc((size_t)wfloats * sizeof(float));
		/* the device batch: rows of all images as one tall frame for the shifts, one launch per step */
		int k0 = dwt_hip_get_option("stat_launches");
		bad |= dwt_hip_shift(d, stride_x, stride_y, W, BATCH * H, -low);
		bad |= dwt_hip_map_batch(DWT_HIP_MAP_LOG, d, image, BATCH, stride_x, W, H, eps);
		shaping += dwt_hip_get_option("stat_launches") - k0;
		bad |= dwt_hip_eaw53_2d_batch(0, d, image, BATCH, stride_x, W, H, &J, 0, dw, wfloats, alpha);
		fill_detail(ops, params, J, DWT_HIP_BAND_COMPRESS, beta);
		k0 = dwt_hip_get_option("stat_launches");
		bad |= dwt_hip_bands_apply_batch(d, image, BATCH, stride_x, W, H, J, ops, params, 0);
		shaping += dwt_hip_get_option("stat_launches") - k0;
		bad |= dwt_hip_eaw53_2d_batch(1, d, image, BATCH, stride_x, W, H, &J, 0, dw, wfloats, alpha);
		k0 = dwt_hip_get_option("stat_launches");
		bad |= dwt_hip_map_batch(DWT_HIP_MAP_EXP, d, image, BATCH, stride_x, W, H, eps);
		bad |= dwt_hip_shift(d, stride_x, stride_y, W, BATCH * H, low);
		shaping += dwt_hip_get_option("stat_launches") - k0;
		if (bad)
			dwt_util_error("hdr flow: %s\n", dwt_hip_last_error());
		/* the host restatement, image by image */
		for (int b = 0; b < BATCH; b++) {
			float *img = host + (size_t)b * W * H;
			int j = -1;
			dwt_util_shift_s(img, W, H, stride_x, stride_y, -low);
			for (size_t i = 0; i < (size_t)W * H; i++)
				img[i] = logf(img[i] + eps);
			if (dwt_hip_eaw53_2d(0, DWT_HIP_EAW_MALLAT, img, stride_x, stride_y, W, H, W, H, &j, 0, 0, hw, alpha))
				dwt_util_error("host forward: %s\n", dwt_hip_last_error());
			each_detail(img, j, compress, beta);
			if (dwt_hip_eaw53_2d(1, DWT_HIP_EAW_MALLAT, img, stride_x, stride_y, W, H, W, H, &j, 0, 0, hw, alpha))
				dwt_util_error("host inverse: %s\n", dwt_hip_last_error());
			for (size_t i = 0; i < (size_t)W * H; i++)
				img[i] = expf(img[i]) - eps;
			dwt_util_shift_s(img, W, H, stride_x, stride_y, low);
		}
		dwt_hip_free(dw);
		free(hw);
		bad = shaping != 5;
	} else {
		float lambda[BATCH];
		/* the batched CDF 9/7 transform takes distinct src and dst: the coefficients live in a second device batch */
		float *c = dwt_hip_malloc(BATCH * image);
		if (!c)
			dwt_util_error("device setup: %s\n", dwt_hip_last_error());
		if (dwt_hip_transform2d_batch(DWT_HIP_CDF97_S, 0, d, c, image, BATCH, stride_x, W, H, &J))
			dwt_util_error("forward: %s\n", dwt_hip_last_error());
		if (dwt_hip_universal_threshold_batch(c, image, BATCH, stride_x, W, H, lambda))
			dwt_util_error("threshold: %s\n", dwt_hip_last_error());
		const int ns = dwt_hip_band_slots(J);
		int *tops = malloc((size_t)BATCH * ns * sizeof(int));
		float *tparams = malloc((size_t)BATCH * ns * sizeof(float));
		for (int b = 0; b < BATCH; b++) /* every image its own threshold: per-image tables, still one launch */
			fill_detail(tops + b * ns, tparams + b * ns, J, DWT_HIP_BAND_SOFT, lambda[b]);
		const int k0 = dwt_hip_get_option("stat_launches");
		if (dwt_hip_bands_apply_batch(c, image, BATCH, stride_x, W, H, J, tops, tparams, ns))
			dwt_util_error("shrinkage: %s\n", dwt_hip_last_error());
		shaping = dwt_hip_get_option("stat_launches") - k0;
		if (dwt_hip_transform2d_batch(DWT_HIP_CDF97_S, 1, c, d, image, BATCH, stride_x, W, H, &J))
			dwt_util_error("inverse: %s\n", dwt_hip_last_error());
		dwt_hip_free(c);
		for (int b = 0; b < BATCH; b++) {
			float *img = host + (size_t)b * W * H;
			int j = -1;
			dwt_cdf97_2f_s(img, stride_x, stride_y, W, H, W, H, &j, 0, 0);
			/* the median magnitude of HH(1) on a copy, as dwt_util_abs_s + dwt_util_band_med_s take it */
			void *p;
			int sx, sy;
			dwt_util_subband_s(img, stride_x, stride_y, W, H, W, H, 1, DWT_HH, &p, &sx, &sy);
			float *mag = malloc((size_t)sx * sy * sizeof(float));
			for (int y = 0; y < sy; y++)
				memcpy(mag + (size_t)y * sx, (char *)p + (size_t)y * stride_x, (size_t)sx * sizeof(float));
			dwt_util_abs_s(mag, sx * stride_y, stride_y, sx, sy);
			const float sigma = dwt_util_band_med_s(mag, sx * stride_y, stride_y, sx, sy) / 0.6745f;
			const float t = sigma * sqrtf(2.f * logf((float)(W * H)));
			free(mag);
			bad |= t != lambda[b];
			dwt_util_log(LOG_INFO, "image %d: threshold %g (host %g)\n", b, lambda[b], t);
			each_detail(img, j, soft, t);
			dwt_cdf97_2i_s(img, stride_x, stride_y, W, H, W, H, j, 0, 0);
		}
		free(tops), free(tparams);
		bad |= shaping != 1;
	}
	const int launches = dwt_hip_get_option("stat_launches") - launches0;
	if (dwt_hip_memcpy_d2h(out, d, BATCH * image))
		dwt_util_error("download: %s\n", dwt_hip_last_error());
	double worst = 0, scale = 0;
	for (size_t i = 0; i < (size_t)BATCH * W * H; i++) {
		const double e = fabs((double)out[i] - host[i]);
		worst = e > worst ? e : worst;
		scale = fabs(host[i]) > scale ? fabs(host[i]) : scale;
	}
	dwt_util_log(LOG_INFO, "%d images of %d x %d, %d levels: %d launches on the device batch, %d of them between the transforms\n", BATCH, W, H, J,
		launches, shaping);
	dwt_util_log(LOG_INFO, "max difference to the host restatement: %g (largest value %g)\n", worst, scale);
	bad |= !(worst <= 1e-4 * scale);
	dwt_util_log(LOG_INFO, bad ? "failure\n" : "success\n");
	dwt_hip_free(d);
	free(in), free(host), free(out);
	dwt_util_finish();
	return bad;
}
