/*
 * lossless16.c -- the reversible int16 CDF 5/3 transform in JPEG 2000 order (dwt_cdf53_2f_i16 / dwt_cdf53_2i_i16, an
 * extension of this library: libdwt has the transform as a single-level core only).  Loads an ASCII PGM into int16
 * samples -- or fills a test pattern --, runs the forward transform, writes a view of the coefficients, runs the inverse
 * and compares sample by sample: the round trip is exact for every int16 image.  Then the same on a device-resident
 * image.  Own code written against include/libdwt.h.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/lossless16.c -o lossless16 \
 *       -Llibdwt_amd -l:libdwt_hip.so -Wl,-rpath,$PWD/libdwt_amd -lm
 *   ./lossless16 [input.pgm [view.pgm]]
 */
#include "libdwt.h"
#include "libdwt_hip.h"

#include <stdlib.h>
#include <string.h>

/* samples that differ between two int16 images of the same layout */
static long differ(const void *a, const void *b, int stride_x, int stride_y, int size_x, int size_y)
{
	long n = 0;
	for (int y = 0; y < size_y; y++)
		for (int x = 0; x < size_x; x++) {
			int16_t p, q;
			memcpy(&p, (const char *)a + (long)y * stride_x + (long)x * stride_y, 2);
			memcpy(&q, (const char *)b + (long)y * stride_x + (long)x * stride_y, 2);
			n += p != q;
		}
	return n;
}

int main(int argc, char **argv)
{
	dwt_util_init();
	dwt_util_log(LOG_INFO, "library: %s on %s\n", dwt_util_version(), dwt_hip_device_name());

	/* host image: from a file (12-bit grey levels), or the reference's pattern */
	int x = 509, y = 381, stride_x, stride_y;
	void *a = NULL, *b = NULL, *v = NULL;
	if (argc > 1) {
		if (dwt_util_load_from_pgm_i16(argv[1], 4095, &a, &stride_x, &stride_y, &x, &y))
			dwt_util_error("cannot load %s\n", argv[1]);
	} else {
		stride_y = sizeof(int16_t);
		stride_x = dwt_util_get_opt_stride(stride_y * x);
		dwt_util_alloc_image(&a, stride_x, stride_y, x, y);
		dwt_util_test_image_fill2_i16(a, stride_x, stride_y, x, y, 0, 0);
	}
	dwt_util_alloc_image(&b, stride_x, stride_y, x, y);
	dwt_util_alloc_image(&v, stride_x, stride_y, x, y);
	memcpy(b, a, dwt_util_image_size(stride_x, stride_y, x, y));

	int j = -1;
	dwt_cdf53_2f_i16(a, stride_x, stride_y, x, y, x, y, &j, 0, 0);
	dwt_util_log(LOG_INFO, "host image %dx%d pitch %d: %d levels\n", x, y, stride_x, j);
	if (argc > 2) {
		dwt_util_conv_show_i16(a, v, stride_x, stride_y, x, y);
		dwt_util_save_to_pgm_i16(argv[2], 255, v, stride_x, stride_y, x, y);
	}
	dwt_cdf53_2i_i16(a, stride_x, stride_y, x, y, x, y, j, 0, 0);
	const long bad_host = differ(a, b, stride_x, stride_y, x, y);
	dwt_util_log(LOG_INFO, bad_host ? "host round trip: images differ\n" : "host round trip: success\n");

	/* device-resident image over the whole int16 range, the same entries */
	const int n = 1024;
	const size_t bytes = (size_t)n * n * sizeof(int16_t);
	int16_t *h = malloc(bytes), *r = malloc(bytes);
	void *d = dwt_hip_malloc(bytes);
	if (!h || !r || !d)
		dwt_util_error("allocation failed: %s\n", dwt_hip_last_error());
	unsigned s = 12345;
	for (size_t i = 0; i < (size_t)n * n; i++) {
		s = s * 1664525u + 1013904223u;
		h[i] = (int16_t)(s >> 16);
	}
	dwt_hip_memcpy_h2d(d, h, bytes);
	j = 5;
	dwt_cdf53_2f_i16(d, n * 2, 2, n, n, n, n, &j, 0, 0);
	dwt_cdf53_2i_i16(d, n * 2, 2, n, n, n, n, j, 0, 0);
	dwt_hip_memcpy_d2h(r, d, bytes);
	const long bad_dev = differ(r, h, n * 2, 2, n, n);
	dwt_util_log(LOG_INFO, bad_dev ? "device round trip: images differ\n" : "device round trip: success\n");

	dwt_hip_free(d);
	free(h);
	free(r);
	dwt_util_free_image(&a);
	dwt_util_free_image(&b);
	dwt_util_free_image(&v);
	dwt_util_finish();
	return bad_host || bad_dev;
}
