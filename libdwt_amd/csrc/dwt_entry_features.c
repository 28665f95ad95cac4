/*
 * dwt_entry_features.c -- libdwt's feature-vector entry points (src/libdwt.h:2875-3309; src/libdwt.c:23086-23786) and
 * dwt_util_abs_s (:24335) as thin C wrappers over dwt_hip_features2d / dwt_hip_band_feature / dwt_hip_abs
 * (include/libdwt_hip.h).  The image may be host or device memory; the vector is host memory, as in the reference.
 * A call that cannot run on the device logs the reason and aborts through dwt_util_error.
 */
#include "../../include/libdwt.h"
#include "../../include/libdwt_hip.h"

#include <math.h>
#include <stdlib.h>

/* src/libdwt.c:20921 */
void dwt_util_subband_const_s(const void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y, int size_i_big_x,
	int size_i_big_y, int j_max, enum dwt_subbands band, const void **dst_ptr, int *dst_size_x, int *dst_size_y)
{
	void *p = NULL;
	dwt_util_subband((void *)ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y, j_max, band, &p, dst_size_x,
		dst_size_y);
	*dst_ptr = p;
}

/* src/libdwt.c:23167 */
int dwt_util_count_subbands_s(const void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y, int size_i_big_x,
	int size_i_big_y, int j_max)
{
	(void)ptr, (void)stride_x, (void)stride_y;
	const int n = dwt_hip_count_subbands(size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y, j_max);
	if (n < 0)
		dwt_util_error("%s: bad sizes\n", __func__);
	return n;
}

/* one feature of every band; fv is host memory wherever the image lies */
static void feature_vector(int feature, const void *ptr, int stride_x, int stride_y, int sox, int soy, int six, int siy, int j_max, float p,
	float *fv, const char *who)
{
	const int n = dwt_hip_count_subbands(sox, soy, six, siy, j_max);
	if (n < 0)
		dwt_util_error("%s: bad sizes\n", who);
	if (n == 0)
		return;
	if (dwt_hip_features2d_hostfv(DWT_HIP_FEATURE_BIT(feature), ptr, stride_x, stride_y, sox, soy, six, siy, j_max, p, fv))
		dwt_util_error("%s: %s\n", who, dwt_hip_last_error());
}

static float band_feature(int feature, const void *ptr, int stride_x, int stride_y, int size_x, int size_y, int j, float p, const char *who)
{
	float v = 0.f;
	if (dwt_hip_band_feature(feature, ptr, stride_x, stride_y, size_x, size_y, j, p, &v))
		dwt_util_error("%s: %s\n", who, dwt_hip_last_error());
	return v;
}

void dwt_util_wps_s(const void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int j_max, float *fv)
{
	feature_vector(DWT_HIP_FEATURE_WPS, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y, j_max, 2.f, fv, __func__);
}

void dwt_util_maxidx_s(const void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int j_max, float *fv)
{
	feature_vector(DWT_HIP_FEATURE_MAXIDX, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y, j_max, 2.f, fv, __func__);
}

void dwt_util_mean_s(const void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int j_max, float *fv)
{
	feature_vector(DWT_HIP_FEATURE_MEAN, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y, j_max, 2.f, fv, __func__);
}

void dwt_util_med_s(const void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int j_max, float *fv)
{
	feature_vector(DWT_HIP_FEATURE_MED, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y, j_max, 2.f, fv, __func__);
}

void dwt_util_var_s(const void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int j_max, float *fv)
{
	feature_vector(DWT_HIP_FEATURE_VAR, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y, j_max, 2.f, fv, __func__);
}

void dwt_util_stdev_s(const void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int j_max, float *fv)
{
	feature_vector(DWT_HIP_FEATURE_STDEV, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y, j_max, 2.f, fv, __func__);
}

void dwt_util_skew_s(const void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int j_max, float *fv)
{
	feature_vector(DWT_HIP_FEATURE_SKEW, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y, j_max, 2.f, fv, __func__);
}

void dwt_util_kurt_s(const void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int j_max, float *fv)
{
	feature_vector(DWT_HIP_FEATURE_KURT, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y, j_max, 2.f, fv, __func__);
}

void dwt_util_maxnorm_s(const void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int j_max, float *fv)
{
	feature_vector(DWT_HIP_FEATURE_MAXNORM, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y, j_max, 2.f, fv, __func__);
}

void dwt_util_norm_s(const void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int j_max, float *fv)
{
	feature_vector(DWT_HIP_FEATURE_NORM, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y, j_max, 2.f, fv, __func__);
}

void dwt_util_lpnorm_s(const void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int j_max, float *fv, float p)
{
	feature_vector(DWT_HIP_FEATURE_LPNORM, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y, j_max, p, fv, __func__);
}

float dwt_util_band_wps_s(const void *ptr, int stride_x, int stride_y, int size_x, int size_y, int j)
{
	return band_feature(DWT_HIP_FEATURE_WPS, ptr, stride_x, stride_y, size_x, size_y, j, 2.f, __func__);
}

float dwt_util_band_maxidx_s(const void *ptr, int stride_x, int stride_y, int size_x, int size_y)
{
	return band_feature(DWT_HIP_FEATURE_MAXIDX, ptr, stride_x, stride_y, size_x, size_y, 0, 2.f, __func__);
}

float dwt_util_band_mean_s(const void *ptr, int stride_x, int stride_y, int size_x, int size_y)
{
	return band_feature(DWT_HIP_FEATURE_MEAN, ptr, stride_x, stride_y, size_x, size_y, 0, 2.f, __func__);
}

float dwt_util_band_med_s(const void *ptr, int stride_x, int stride_y, int size_x, int size_y)
{
	return band_feature(DWT_HIP_FEATURE_MED, ptr, stride_x, stride_y, size_x, size_y, 0, 2.f, __func__);
}

float dwt_util_band_var_s(const void *ptr, int stride_x, int stride_y, int size_x, int size_y)
{
	return band_feature(DWT_HIP_FEATURE_VAR, ptr, stride_x, stride_y, size_x, size_y, 0, 2.f, __func__);
}

float dwt_util_band_stdev_s(const void *ptr, int stride_x, int stride_y, int size_x, int size_y)
{
	return band_feature(DWT_HIP_FEATURE_STDEV, ptr, stride_x, stride_y, size_x, size_y, 0, 2.f, __func__);
}

float dwt_util_band_skew_s(const void *ptr, int stride_x, int stride_y, int size_x, int size_y)
{
	return band_feature(DWT_HIP_FEATURE_SKEW, ptr, stride_x, stride_y, size_x, size_y, 0, 2.f, __func__);
}

float dwt_util_band_kurt_s(const void *ptr, int stride_x, int stride_y, int size_x, int size_y)
{
	return band_feature(DWT_HIP_FEATURE_KURT, ptr, stride_x, stride_y, size_x, size_y, 0, 2.f, __func__);
}

float dwt_util_band_maxnorm_s(const void *ptr, int stride_x, int stride_y, int size_x, int size_y)
{
	return band_feature(DWT_HIP_FEATURE_MAXNORM, ptr, stride_x, stride_y, size_x, size_y, 0, 2.f, __func__);
}

float dwt_util_band_norm_s(const void *ptr, int stride_x, int stride_y, int size_x, int size_y)
{
	return band_feature(DWT_HIP_FEATURE_NORM, ptr, stride_x, stride_y, size_x, size_y, 0, 2.f, __func__);
}

float dwt_util_band_lpnorm_s(const void *ptr, int stride_x, int stride_y, int size_x, int size_y, float p)
{
	return band_feature(DWT_HIP_FEATURE_LPNORM, ptr, stride_x, stride_y, size_x, size_y, 0, p, __func__);
}

/* src/libdwt.c:23343 */
float dwt_util_band_moment_s(const void *ptr, int stride_x, int stride_y, int size_x, int size_y, int n, float c)
{
	float v = 0.f;
	if (dwt_hip_band_moment(ptr, stride_x, stride_y, size_x, size_y, n, 0, c, &v))
		dwt_util_error("%s: %s\n", __func__, dwt_hip_last_error());
	return v;
}

/* src/libdwt.c:23372 */
float dwt_util_band_cmoment_s(const void *ptr, int stride_x, int stride_y, int size_x, int size_y, int n)
{
	float v = 0.f;
	if (dwt_hip_band_moment(ptr, stride_x, stride_y, size_x, size_y, n, 1, 0.f, &v))
		dwt_util_error("%s: %s\n", __func__, dwt_hip_last_error());
	return v;
}

/* src/libdwt.c:23412: the central moment over powf(stdev, n) */
float dwt_util_band_smoment_s(const void *ptr, int stride_x, int stride_y, int size_x, int size_y, int n)
{
	const float stdev = dwt_util_band_stdev_s(ptr, stride_x, stride_y, size_x, size_y);
	return dwt_util_band_cmoment_s(ptr, stride_x, stride_y, size_x, size_y, n) / powf(stdev, n);
}

/* src/libdwt.c:24335 */
void dwt_util_abs_s(void *ptr, int stride_x, int stride_y, int size_x, int size_y)
{
	if (dwt_hip_abs(ptr, stride_x, stride_y, size_x, size_y))
		dwt_util_error("%s: %s\n", __func__, dwt_hip_last_error());
}
