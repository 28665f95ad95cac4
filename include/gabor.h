/*
 * gabor.h -- the time-frequency entries of libdwt (src/gabor.h), served by libdwt_hip.so.
 *
 * gabor_ft_s (short-time Fourier transform, Gaussian window), gabor_wt_s (continuous wavelet transform, complex Morlet
 * wavelet) and gabor_st_s (S transform) correlate a real signal of sig_size samples, sig_stride bytes apart, with `bins`
 * complex kernels and store the magnitudes -- their _arg_ twins the arguments -- into a plane of `bins` rows: element
 * (row, t) at plane + row*stride_x + t*stride_y, bin y in row bins-1-y.  timefreq_line / timefreq_arg_line do one row
 * with a kernel the caller brings; dwt_util_cdot1_s is one sample of it, as a complex number.  phase_derivative_s and
 * detect_ridges{1,2,3}_s run over such planes.  Signals and planes are host memory or device memory alike; kernels are
 * host memory.  Batches of signals against one resident bank of kernels: dwt_hip_timefreq_batch (libdwt_hip.h).
 *
 * All but dwt_util_cdot1_s are inline wrappers over dwt_hip_* functions: the library's C symbols all carry its own
 * prefixes, and a program written against the reference's gabor.h compiles and links against libdwt_hip.so unchanged.
 * As for the other entries, a call that cannot run on the device logs the reason and aborts through dwt_util_error.
 * The generators (gabor_function, gabor_wavelet, gaussian_size, gaussian_center, gabor_gen_kernel) run on the host.
 */
#ifndef GABOR_H
#define GABOR_H

#ifndef __cplusplus
#include <complex.h>
#endif
#include <stdlib.h>

#include "libdwt.h"
#include "libdwt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sum of func[func_center + i] * conj(kern[kern_center + i]) over the i both hold, ascending */
float _Complex dwt_util_cdot1_s(const float *func, int func_size, int func_stride, int func_center, const float _Complex *kern,
	int kern_size, int kern_stride, int kern_center);

static inline float _Complex gabor_wavelet(float t, float sigma, float f, float a)
{
	union {
		float v[2];
		float _Complex z;
	} u;
	dwt_hip_gabor_wavelet(t, sigma, f, a, u.v);
	return u.z;
}

static inline float _Complex gabor_function(float t, float sigma, float f)
{
	return gabor_wavelet(t, sigma, f, 1.f);
}

static inline int gaussian_size(float sigma, float a)
{
	return dwt_hip_gaussian_size(sigma, a);
}

static inline int gaussian_center(float sigma, float a)
{
	return dwt_hip_gaussian_size(sigma, a) / 2;
}

/* *ckern is reallocated to gaussian_size(sigma, a) elements `stride` bytes apart and filled */
static inline void gabor_gen_kernel(float _Complex **ckern, int stride, float sigma, float freq, float a)
{
	*ckern = (float _Complex *)realloc(*ckern, (size_t)stride * (size_t)dwt_hip_gaussian_size(sigma, a));
	dwt_hip_gabor_gen_kernel(*ckern, stride, sigma, freq, a);
}

static inline void timefreq_line(float *dst, int dst_stride, const float *src, int src_stride, int size, const float _Complex *kern,
	int kern_stride, int kern_size, int kern_center)
{
	if (dwt_hip_timefreq_line(0, dst, dst_stride, src, src_stride, size, kern, kern_stride, kern_size, kern_center))
		dwt_util_error("timefreq_line: %s\n", dwt_hip_last_error());
}

static inline void timefreq_arg_line(float *dst, int dst_stride, const float *src, int src_stride, int size, const float _Complex *kern,
	int kern_stride, int kern_size, int kern_center)
{
	if (dwt_hip_timefreq_line(1, dst, dst_stride, src, src_stride, size, kern, kern_stride, kern_size, kern_center))
		dwt_util_error("timefreq_arg_line: %s\n", dwt_hip_last_error());
}

static inline void gabor_ft_s(const float *sig, int sig_stride, int sig_size, void *plane, int stride_x, int stride_y, int bins, float sigma)
{
	if (dwt_hip_gabor_transform(DWT_HIP_TIMEFREQ_FT, 0, sig, sig_stride, sig_size, plane, stride_x, stride_y, bins, sigma, 0.f))
		dwt_util_error("gabor_ft_s: %s\n", dwt_hip_last_error());
}

static inline void gabor_ft_arg_s(const float *sig, int sig_stride, int sig_size, void *plane, int stride_x, int stride_y, int bins, float sigma)
{
	if (dwt_hip_gabor_transform(DWT_HIP_TIMEFREQ_FT, 1, sig, sig_stride, sig_size, plane, stride_x, stride_y, bins, sigma, 0.f))
		dwt_util_error("gabor_ft_arg_s: %s\n", dwt_hip_last_error());
}

static inline void gabor_wt_s(const float *sig, int sig_stride, int sig_size, void *plane, int stride_x, int stride_y, int bins, float sigma,
	float freq)
{
	if (dwt_hip_gabor_transform(DWT_HIP_TIMEFREQ_WT, 0, sig, sig_stride, sig_size, plane, stride_x, stride_y, bins, sigma, freq))
		dwt_util_error("gabor_wt_s: %s\n", dwt_hip_last_error());
}

static inline void gabor_wt_arg_s(const float *sig, int sig_stride, int sig_size, void *plane, int stride_x, int stride_y, int bins, float sigma,
	float freq)
{
	if (dwt_hip_gabor_transform(DWT_HIP_TIMEFREQ_WT, 1, sig, sig_stride, sig_size, plane, stride_x, stride_y, bins, sigma, freq))
		dwt_util_error("gabor_wt_arg_s: %s\n", dwt_hip_last_error());
}

static inline void gabor_st_s(const float *sig, int sig_stride, int sig_size, void *plane, int stride_x, int stride_y, int bins)
{
	if (dwt_hip_gabor_transform(DWT_HIP_TIMEFREQ_ST, 0, sig, sig_stride, sig_size, plane, stride_x, stride_y, bins, 0.f, 0.f))
		dwt_util_error("gabor_st_s: %s\n", dwt_hip_last_error());
}

static inline void gabor_st_arg_s(const float *sig, int sig_stride, int sig_size, void *plane, int stride_x, int stride_y, int bins)
{
	if (dwt_hip_gabor_transform(DWT_HIP_TIMEFREQ_ST, 1, sig, sig_stride, sig_size, plane, stride_x, stride_y, bins, 0.f, 0.f))
		dwt_util_error("gabor_st_arg_s: %s\n", dwt_hip_last_error());
}

/* the difference of neighbouring angles along x, wrapped by 2 pi into [-limit, +limit] */
static inline void phase_derivative_s(const void *angle, void *derivative, int stride_x, int stride_y, int size_x, int size_y, float limit)
{
	if (dwt_hip_phase_derivative(angle, derivative, stride_x, stride_y, size_x, size_y, 1, 0, limit))
		dwt_util_error("phase_derivative_s: %s\n", dwt_hip_last_error());
}

/* local maxima of the magnitude along x, above the threshold */
static inline void detect_ridges1_s(const void *magnitude, void *ridges, int stride_x, int stride_y, int size_x, int size_y, float threshold)
{
	if (dwt_hip_detect_ridges(1, magnitude, ridges, stride_x, stride_y, size_x, size_y, 1, 0, threshold))
		dwt_util_error("detect_ridges1_s: %s\n", dwt_hip_last_error());
}

/* negative phase derivative beyond the threshold */
static inline void detect_ridges2_s(const void *inst_freq, void *ridges, int stride_x, int stride_y, int size_x, int size_y, float threshold)
{
	if (dwt_hip_detect_ridges(2, inst_freq, ridges, stride_x, stride_y, size_x, size_y, 1, 0, threshold))
		dwt_util_error("detect_ridges2_s: %s\n", dwt_hip_last_error());
}

/* maxima of the magnitude in the direction of its gradient, above the threshold */
static inline void detect_ridges3_s(const void *magnitude, void *ridges, int stride_x, int stride_y, int size_x, int size_y, float threshold)
{
	if (dwt_hip_detect_ridges(3, magnitude, ridges, stride_x, stride_y, size_x, size_y, 1, 0, threshold))
		dwt_util_error("detect_ridges3_s: %s\n", dwt_hip_last_error());
}

#ifdef __cplusplus
}
#endif
#endif
