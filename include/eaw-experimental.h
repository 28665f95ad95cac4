/*
 * eaw-experimental.h -- the edge-avoiding CDF 9/7 wavelet entries of libdwt (src/eaw-experimental.h, "WCDF 9/7"), served
 * by libdwt_hip.so.
 *
 * The lifting scheme of the CDF 9/7 wavelet with Fattal's edge-avoiding weights: every pass over a line computes
 * w[i] = 1 / (|x[i] - x[i+1]|^alpha + 1e-5) from its input and runs predict 1, update 1, predict 2 and update 2 as
 * weighted averages of the two neighbours with those weights, then scales.  The image is transformed in place in the
 * Mallat layout, rows then columns per level; the inverse runs columns then rows with the forward's weights.  `ptr` is
 * host or device memory with any byte strides.  Arguments, level clamp, decompose_one and zero_padding are those of
 * dwt_eaw53_2f_s / dwt_eaw53_2i_s (libdwt.h).  alpha 1 and 0 give the reference's bits; any other alpha is within 1 ulp
 * in the weights (libdwt_hip.h).  A call that cannot run on the device logs the reason and aborts through dwt_util_error.
 * Device-resident weights and batches: dwt_hip_eaw97_2d, dwt_hip_eaw97_2d_batch (libdwt_hip.h).
 */
#ifndef EAW_EXPERIMENTAL_H
#define EAW_EXPERIMENTAL_H

#ifdef __cplusplus
extern "C" {
#endif

/* Forward.  Allocates wH[j] (size_o_src_y x size_i_src_x, row-major) and wV[j] (size_o_src_x x size_i_src_y,
 * column-major) of every level j < *j_max_ptr (after the clamp) with dwt_util_alloc: host memory the caller frees with
 * free().  Entries of one-sample lines are not written. */
void dwt_eaw97_2f_s(void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int *j_max_ptr, int decompose_one, int zero_padding,
	float *wH[], float *wV[], float alpha);

/* Inverse of the above with the forward's weights (host arrays). */
void dwt_eaw97_2i_s(void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int j_max, int decompose_one, int zero_padding,
	float *wH[], float *wV[]);

#ifdef __cplusplus
}
#endif
#endif
