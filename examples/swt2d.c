/*
 * swt2d.c -- the undecimated (stationary) CDF 9/7 pyramid of a small batch of images resident in device memory: one
 * dwt_hip_swt2d_batch call, three levels, every plane the size of the image -- HL, LH and HH of every level and the last
 * level's LL.  Prints one checksum per plane (the sum of the coefficients' bit patterns modulo 2^32, which no order of
 * summation changes) and the number of kernel launches the call took: one per level.  The images are seeded noise; no
 * input file is read.  Own code written against include/.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/swt2d.c -o swt2d -Llibdwt_amd -l:libdwt_hip.so -Wl,-rpath,$PWD/libdwt_amd -lm
 */
#include "libdwt.h"
#include "libdwt_hip.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static unsigned rnd(unsigned *s) /* a small LCG: the same images everywhere */
{
	*s = *s * 1664525u + 1013904223u;
	return *s >> 8;
}

static unsigned checksum(const float *p, size_t n)
{
	unsigned sum = 0;
	for (size_t i = 0; i < n; i++) {
		uint32_t bits;
		memcpy(&bits, p + i, sizeof bits);
		sum += bits;
	}
	return sum;
}

int main(void)
{
	dwt_util_init();
	dwt_util_log(LOG_INFO, "library: %s on %s\n", dwt_util_version(), dwt_hip_device_name());

	enum { batch = 2, size_x = 70, size_y = 48, levels = 3 };
	const size_t plane = (size_t)size_x * size_y, plane_bytes = plane * sizeof(float);
	/* per image: HL, LH, HH of every level, then the last level's LL */
	enum { per_image = 3 * levels + 1 };
	const size_t src_bytes = batch * plane_bytes, out_bytes = (size_t)batch * per_image * plane_bytes;
	float *img = malloc(src_bytes), *out = malloc(out_bytes);
	unsigned seed = 2024;
	for (size_t i = 0; i < batch * plane; i++)
		img[i] = (float)(rnd(&seed) & 0xffff) / 65536.f - 0.5f;

	float *d_img = dwt_hip_malloc(src_bytes), *d_out = dwt_hip_malloc(out_bytes);
	if (!d_img || !d_out || dwt_hip_memcpy_h2d(d_img, img, src_bytes))
		dwt_util_error("device setup: %s\n", dwt_hip_last_error());
	const int launches0 = dwt_hip_get_option("stat_launches");
	/* dst_h and dst_l share the batch stride: detail band k of level l of image b at plane b * per_image + 3 * l + k - 1, the
	 * last LL behind them at plane b * per_image + 3 * levels */
	if (dwt_hip_swt2d_batch(DWT_HIP_CDF97_S, d_img, plane_bytes, batch, size_x * sizeof(float), sizeof(float), size_x, size_y, levels, d_out,
		    d_out + 3 * levels * plane, 1, per_image * plane_bytes, plane_bytes, size_x * sizeof(float)))
		dwt_util_error("dwt_hip_swt2d_batch: %s\n", dwt_hip_last_error());
	const int launches = dwt_hip_get_option("stat_launches") - launches0;
	if (dwt_hip_memcpy_d2h(out, d_out, out_bytes))
		dwt_util_error("download: %s\n", dwt_hip_last_error());

	static const char *const band[3] = {"HL", "LH", "HH"};
	for (int b = 0; b < batch; b++) {
		for (int lev = 0; lev < levels; lev++)
			for (int k = 0; k < 3; k++)
				printf("image %d level %d %s %08x\n", b, lev, band[k], checksum(out + ((size_t)b * per_image + 3 * lev + k) * plane, plane));
		printf("image %d level %d LL %08x\n", b, levels - 1, checksum(out + ((size_t)b * per_image + 3 * levels) * plane, plane));
	}
	printf("%d images of %d x %d, %d levels: %d launch(es)\n", batch, size_x, size_y, levels, launches);

	dwt_hip_free(d_img);
	dwt_hip_free(d_out);
	free(img), free(out);
	dwt_util_finish();
	return launches != levels;
}
