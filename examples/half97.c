/*
 * half97.c -- the float CDF 9/7 on IEEE binary16 storage (dwt_cdf97_2f_h / dwt_cdf97_2i_h, an extension of this library).
 * Fills the reference's float test image, converts it to binary16 on the host, uploads it, runs the forward transform and
 * its inverse on the resident half image, downloads it, converts it back to float and prints the maximum error against the
 * input.  The transform is not reversible: every level rounds its result to binary16 once.  Own code
 * written against include/libdwt.h.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/half97.c -o half97 \
 *       -Llibdwt_amd -l:libdwt_hip.so -Wl,-rpath,$PWD/libdwt_amd -lm
 *   ./half97 [levels]
 */
#include "libdwt.h"
#include "libdwt_hip.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

int main(int argc, char **argv)
{
	dwt_util_init();
	dwt_util_log(LOG_INFO, "library: %s on %s\n", dwt_util_version(), dwt_hip_device_name());

	/* the reference's pattern (values in [0, 1]) scaled to 8-bit grey levels */
	const int x = 1024, y = 768;
	const int fstride = x * (int)sizeof(float), hstride = x * 2;
	float *a = malloc((size_t)fstride * y), *b = malloc((size_t)fstride * y);
	uint16_t *h = malloc((size_t)hstride * y);
	void *d = dwt_hip_malloc((size_t)hstride * y);
	if (!a || !b || !h || !d)
		dwt_util_error("allocation failed: %s\n", dwt_hip_last_error());
	dwt_util_test_image_fill_s(a, fstride, sizeof(float), x, y, 0);
	for (long i = 0; i < (long)x * y; i++)
		a[i] = floorf(255.f * a[i] + 0.5f);

	dwt_util_float_to_half(h, hstride, 2, a, fstride, sizeof(float), x, y);
	dwt_hip_memcpy_h2d(d, h, (size_t)hstride * y);
	int j = argc > 1 ? atoi(argv[1]) : 5;
	dwt_cdf97_2f_h(d, hstride, 2, x, y, x, y, &j, 0, 0);
	dwt_cdf97_2i_h(d, hstride, 2, x, y, x, y, j, 0, 0);
	dwt_hip_memcpy_d2h(h, d, (size_t)hstride * y);
	dwt_util_half_to_float(b, fstride, sizeof(float), h, hstride, 2, x, y);

	float err = 0.f;
	for (long i = 0; i < (long)x * y; i++) {
		const float e = fabsf(b[i] - a[i]);
		if (!(e <= err)) /* (a NaN counts) */
			err = e;
	}
	dwt_util_log(LOG_INFO, "%dx%d, %d levels, round trip: maximum error %g grey levels of 255\n", x, y, j, err);

	dwt_hip_free(d);
	free(a);
	free(b);
	free(h);
	dwt_util_finish();
	return !(err <= 1.0f);
}
