/*
 * dwt_entry_condition.c -- libdwt's conditioning entry points of the spectra programs (src/libdwt.c:25426-26055):
 * dwt_util_shift21_med_s, _center21_s, _center1_s, _get_center1_s, _displace1_s, _displace1_zero_s, _scale21_s, _shift_s,
 * _scale_s, _find_min_max_s as thin C wrappers over dwt_hip_rows_* / dwt_hip_shift / dwt_hip_scale (include/libdwt_hip.h),
 * and the two pointer helpers dwt_util_viewport / dwt_util_crop21.  NOTE the reference's argument order here: sizes
 * before strides.  Rows may be host or device memory.  A call that cannot run on the device logs the reason and aborts
 * through dwt_util_error; the reference's per-row warnings become one summary warning.
 */
#include "../../include/libdwt.h"
#include "../../include/libdwt_hip.h"

#include <assert.h>
#include <stdlib.h>

#define TRY(call)                                                                              \
	do {                                                                                       \
		if (call)                                                                              \
			dwt_util_error("%s: %s\n", __func__, dwt_hip_last_error());                        \
	} while (0)

/* the stride between rows is never read for one row: the reference's programs pass 0 there */
static size_t row_stride(int stride_x, int size_y) { return size_y > 1 ? (size_t)stride_x : 0; }

int dwt_util_find_min_max_s(const void *ptr, int size_x, int size_y, int stride_x, int stride_y, float *min, float *max)
{
	assert(ptr && size_x > 0 && size_y > 0);
	float *mn = malloc(2 * sizeof(float) * (size_t)size_y), *mx = mn ? mn + size_y : NULL;
	if (!mn)
		dwt_util_error("%s: out of memory\n", __func__);
	TRY(dwt_hip_rows_min_max(ptr, row_stride(stride_x, size_y), (size_t)stride_y, size_y, size_x, mn, mx));
	*min = mn[0];
	*max = mx[0];
	for (int y = 1; y < size_y; y++) {
		if (mx[y] > *max)
			*max = mx[y];
		if (mn[y] < *min)
			*min = mn[y];
	}
	free(mn);
	return 0;
}

int dwt_util_shift_s(void *ptr, int size_x, int size_y, int stride_x, int stride_y, float a)
{
	TRY(dwt_hip_shift(ptr, stride_x, stride_y, size_x, size_y, a));
	return 0;
}

int dwt_util_scale_s(void *ptr, int size_x, int size_y, int stride_x, int stride_y, float a)
{
	TRY(dwt_hip_scale(ptr, stride_x, stride_y, size_x, size_y, a));
	return 0;
}

int dwt_util_scale21_s(void *ptr, int size_x, int size_y, int stride_x, int stride_y, float lo, float hi)
{
	assert(ptr && hi > lo);
	if (size_y <= 0)
		return 0;
	int *info = malloc(4 * sizeof(int) * (size_t)size_y);
	if (!info)
		dwt_util_error("%s: out of memory\n", __func__);
	TRY(dwt_hip_rows_condition(DWT_HIP_ROWS_SCALE, ptr, row_stride(stride_x, size_y), (size_t)stride_y, size_y, size_x, 0, lo, hi, info));
	int skipped = 0;
	for (int y = 0; y < size_y; y++)
		skipped += info[4 * y + 3];
	free(info);
	if (skipped)
		dwt_util_log(LOG_WARN, "Cannot scale %i of %i rows (min=max)\n", skipped, size_y);
	return 0;
}

int dwt_util_displace1_s(void *ptr, int size_x, int stride_y, int displ_x)
{
	if (displ_x)
		TRY(dwt_hip_rows_displace(ptr, 0, (size_t)stride_y, 1, size_x, NULL, displ_x, 0));
	return 0;
}

int dwt_util_displace1_zero_s(void *ptr, int size_x, int stride_y, int displ_x)
{
	if (displ_x)
		TRY(dwt_hip_rows_displace(ptr, 0, (size_t)stride_y, 1, size_x, NULL, displ_x, 1));
	return 0;
}

/* the reference warns per centre evaluation; here once per call, with the counts */
static void warn_centres(const char *who, int size_y)
{
	int zero_norm = 0, no_index = 0;
	if (dwt_hip_rows_warnings(&zero_norm, &no_index))
		dwt_util_error("%s: %s\n", who, dwt_hip_last_error());
	if (zero_norm)
		dwt_util_log(LOG_WARN, "Cannot get a center of signal due to its zero norm! (%i evaluation(s) over %i row(s))\n", zero_norm, size_y);
	if (no_index)
		dwt_util_log(LOG_WARN, "Cannot found center indexes! (%i evaluation(s) over %i row(s))\n", no_index, size_y);
}

int dwt_util_get_center1_s(const void *ptr, int size_x, int stride_y)
{
	int c = 0;
	TRY(dwt_hip_rows_center_index(ptr, 0, (size_t)stride_y, 1, size_x, &c));
	warn_centres(__func__, 1);
	return c;
}

int dwt_util_center1_s(void *ptr, int size_x, int stride_y, int max_iters)
{
	return dwt_util_center21_s(ptr, size_x, 1, 0, stride_y, max_iters);
}

int dwt_util_center21_s(void *ptr, int size_x, int size_y, int stride_x, int stride_y, int max_iters)
{
	if (size_y > 0 && max_iters > 0) {
		TRY(dwt_hip_rows_condition(DWT_HIP_ROWS_CENTER, ptr, row_stride(stride_x, size_y), (size_t)stride_y, size_y, size_x, max_iters, 0.f, 1.f,
			NULL));
		warn_centres(__func__, size_y);
	}
	return 0;
}

void dwt_util_shift21_med_s(void *ptr, int size_x, int size_y, int stride_x, int stride_y)
{
	if (size_y > 0)
		TRY(dwt_hip_rows_condition(DWT_HIP_ROWS_MED_SHIFT, ptr, row_stride(stride_x, size_y), (size_t)stride_y, size_y, size_x, 0, 0.f, 1.f, NULL));
}

void *dwt_util_viewport(void *ptr, int size_x, int size_y, int stride_x, int stride_y, int offset_x, int offset_y)
{
	assert(offset_x < size_x && offset_y < size_y);
	(void)size_x, (void)size_y;
	return dwt_util_addr_coeff_s(ptr, offset_y, offset_x, stride_x, stride_y);
}

void *dwt_util_crop21(void *ptr, int size_x, int size_y, int stride_x, int stride_y, int len_x)
{
	(void)size_y;
	assert(len_x > 0 && len_x < size_x);
	return dwt_util_addr_coeff_s(ptr, 0, size_x / 2 - len_x / 2, stride_x, stride_y);
}
