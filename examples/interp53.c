/*
 * interp53.c -- the interpolating 5/3 wavelet (CDF 5/3 with the predict step alone) through libdwt's drop-in entries:
 * the flow of libdwt's examples/simple-interpl (512x512 float host image, row pitch from dwt_util_get_opt_stride,
 * full decomposition, inverse, compare), then one round trip of a device-resident image through the same entries.
 * Own code written against include/libdwt.h.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/interp53.c -o interp53 \
 *       -Llibdwt_amd -l:libdwt_hip.so -Wl,-rpath,$PWD/libdwt_amd -lm
 */
#include "libdwt.h"
#include "libdwt_hip.h"

#include <stdlib.h>

int main(void)
{
	dwt_util_init();
	dwt_util_log(LOG_INFO, "library: %s on %s\n", dwt_util_version(), dwt_hip_device_name());

	/* host image, drop-in calls */
	const int x = 512, y = 512;
	const int stride_y = sizeof(float);
	const int stride_x = dwt_util_get_opt_stride(stride_y * x);
	void *a, *b;
	dwt_util_alloc_image(&a, stride_x, stride_y, x, y);
	dwt_util_alloc_image(&b, stride_x, stride_y, x, y);
	dwt_util_test_image_fill_s(a, stride_x, stride_y, x, y, 0);
	dwt_util_copy_s(a, b, stride_x, stride_y, x, y);
	int j = -1;
	dwt_interp53_2f_s(a, stride_x, stride_y, x, y, x, y, &j, 0, 0);
	dwt_util_log(LOG_INFO, "host image %dx%d pitch %d: %d levels\n", x, y, stride_x, j);
	dwt_interp53_2i_s(a, stride_x, stride_y, x, y, x, y, j, 0, 0);
	const int bad_host = dwt_util_compare_s(a, b, stride_x, stride_y, x, y);
	dwt_util_log(LOG_INFO, bad_host ? "host round trip: images differ\n" : "host round trip: success\n");

	/* device-resident image, the same entries */
	const int n = 1024;
	const size_t bytes = (size_t)n * n * sizeof(float);
	float *h = malloc(bytes), *r = malloc(bytes);
	void *d = dwt_hip_malloc(bytes);
	if (!h || !r || !d)
		dwt_util_error("allocation failed: %s\n", dwt_hip_last_error());
	dwt_util_test_image_fill_s(h, n * 4, 4, n, n, 0);
	dwt_hip_memcpy_h2d(d, h, bytes);
	j = 5;
	dwt_interp53_2f_s(d, n * 4, 4, n, n, n, n, &j, 0, 0);
	dwt_interp53_2i_s(d, n * 4, 4, n, n, n, n, j, 0, 0);
	dwt_hip_memcpy_d2h(r, d, bytes);
	const int bad_dev = dwt_util_compare_s(r, h, n * 4, 4, n, n);
	dwt_util_log(LOG_INFO, bad_dev ? "device round trip: images differ\n" : "device round trip: success\n");

	dwt_hip_free(d);
	free(h);
	free(r);
	dwt_util_free_image(&a);
	dwt_util_free_image(&b);
	dwt_util_finish();
	return bad_host || bad_dev;
}
