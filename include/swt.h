/*
 * swt.h -- the stationary wavelet transform entries of libdwt (src/swt.h), served by libdwt_hip.so.
 *
 * One level of the undecimated transform of one line: src is filtered with the low-pass filter into dst_l and with the
 * high-pass filter into dst_h, both filters dilated by 1 << level, borders replicated.  All three have N float elements
 * `stride` bytes apart and must not overlap; they are host memory or device memory alike.  A multi-level transform
 * feeds dst_l of level l to level l + 1.  Batches of lines, every level in one call: dwt_hip_swt1d_batch (libdwt_hip.h).
 *
 * The two entries are inline wrappers over dwt_hip_swt1d_level: the library's C symbols all carry its own prefixes, and
 * a program written against the reference's swt.h compiles and links against libdwt_hip.so unchanged.  As for the
 * other entries, a call that cannot run on the device logs the reason and aborts through dwt_util_error.
 */
#ifndef SWT_H
#define SWT_H

#include "libdwt.h"
#include "libdwt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* CDF 9/7: 9 low-pass and 7 high-pass taps */
static inline void swt_cdf97_f_ex_stride_s(const void *src, void *dst_l, void *dst_h, int N, int stride, int level)
{
	if (dwt_hip_swt1d_level(DWT_HIP_CDF97_S, src, dst_l, dst_h, N, stride, level))
		dwt_util_error("swt_cdf97_f_ex_stride_s: %s\n", dwt_hip_last_error());
}

/* CDF 5/3: 5 low-pass and 3 high-pass taps */
static inline void swt_cdf53_f_ex_stride_s(const void *src, void *dst_l, void *dst_h, int N, int stride, int level)
{
	if (dwt_hip_swt1d_level(DWT_HIP_CDF53_S, src, dst_l, dst_h, N, stride, level))
		dwt_util_error("swt_cdf53_f_ex_stride_s: %s\n", dwt_hip_last_error());
}

#ifdef __cplusplus
}
#endif
#endif
