/*
 * dwt_entry_1d.c -- libdwt's 1-D entry points (src/libdwt.h:1128-1262, 1160, 1217) as thin C wrappers over
 * dwt_hip_transform1d_batch (include/libdwt_hip.h).  As for the 2-D entries (dwt_entry.c), a call that cannot run
 * on the device logs the reason and aborts through dwt_util_error.
 */
#include "../../include/libdwt.h"
#include "../../include/libdwt_hip.h"

#include <stddef.h>

static void run1d(int wavelet, int inverse, void *ptr, size_t line_stride, int stride_y, int n_lines, int sox, int six,
	int *j, int zero_padding, const char *who)
{
	if (dwt_hip_transform1d_batch(wavelet, inverse, ptr, ptr, line_stride, stride_y, n_lines, sox, six, j, zero_padding))
		dwt_util_error("%s: %s\n", who, dwt_hip_last_error());
}

/* src/libdwt.c:16025 */
void dwt_cdf97_1f_s(void *ptr, int stride_y, int size_o_big_x, int size_i_big_x, int *j_max_ptr, int zero_padding)
{
	run1d(DWT_HIP_CDF97_S, 0, ptr, 0, stride_y, 1, size_o_big_x, size_i_big_x, j_max_ptr, zero_padding, __func__);
}

/* src/libdwt.c:16097 */
void dwt_cdf53_1f_s(void *ptr, int stride_y, int size_o_big_x, int size_i_big_x, int *j_max_ptr, int zero_padding)
{
	run1d(DWT_HIP_CDF53_S, 0, ptr, 0, stride_y, 1, size_o_big_x, size_i_big_x, j_max_ptr, zero_padding, __func__);
}

/* src/libdwt.c:15766 */
void dwt_cdf97_1i_s(void *ptr, int stride_y, int size_o_big_x, int size_i_big_x, int j_max, int zero_padding)
{
	run1d(DWT_HIP_CDF97_S, 1, ptr, 0, stride_y, 1, size_o_big_x, size_i_big_x, &j_max, zero_padding, __func__);
}

/* src/libdwt.c:15835 */
void dwt_cdf53_1i_s(void *ptr, int stride_y, int size_o_big_x, int size_i_big_x, int j_max, int zero_padding)
{
	run1d(DWT_HIP_CDF53_S, 1, ptr, 0, stride_y, 1, size_o_big_x, size_i_big_x, &j_max, zero_padding, __func__);
}

/* src/libdwt.c:16166 */
void dwt_interp53_1f_s(void *ptr, int stride_y, int size_o_big_x, int size_i_big_x, int *j_max_ptr, int zero_padding)
{
	run1d(DWT_HIP_INTERP53_S, 0, ptr, 0, stride_y, 1, size_o_big_x, size_i_big_x, j_max_ptr, zero_padding, __func__);
}

/* src/libdwt.c:15900 */
void dwt_interp53_1i_s(void *ptr, int stride_y, int size_o_big_x, int size_i_big_x, int j_max, int zero_padding)
{
	run1d(DWT_HIP_INTERP53_S, 1, ptr, 0, stride_y, 1, size_o_big_x, size_i_big_x, &j_max, zero_padding, __func__);
}

/* src/libdwt.c:15965: the reference calls dwt_cdf97_1f_s row by row with the same j_max_ptr (the first row clamps
 * it); here one batched call.  No rows: *j_max_ptr untouched. */
void dwt_cdf97_2f1_s(void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y, int size_i_big_x,
	int size_i_big_y, int *j_max_ptr, int zero_padding)
{
	(void)size_o_big_y;
	if (size_i_big_y > 0)
		run1d(DWT_HIP_CDF97_S, 0, ptr, (size_t)(long)stride_x, stride_y, size_i_big_y, size_o_big_x, size_i_big_x, j_max_ptr,
			zero_padding, __func__);
}

/* src/libdwt.c:15995 */
void dwt_cdf53_2f1_s(void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y, int size_i_big_x,
	int size_i_big_y, int *j_max_ptr, int zero_padding)
{
	(void)size_o_big_y;
	if (size_i_big_y > 0)
		run1d(DWT_HIP_CDF53_S, 0, ptr, (size_t)(long)stride_x, stride_y, size_i_big_y, size_o_big_x, size_i_big_x, j_max_ptr,
			zero_padding, __func__);
}
