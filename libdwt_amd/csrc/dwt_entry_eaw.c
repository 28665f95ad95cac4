/*
 * dwt_entry_eaw.c -- libdwt's edge-avoiding entry points, 5/3 (src/libdwt.h:742-796, 1073-1100) and 9/7
 * (src/eaw-experimental.h), as thin C wrappers over dwt_hip_eaw53_2d / dwt_hip_eaw97_2d (include/libdwt_hip.h), and
 * dwt_util_alloc.  The weights cross as one buffer in the image's memory space; the forward hands them out as the
 * reference does, one dwt_util_alloc'd host array per level and direction.  A call that cannot run on the device logs
 * the reason and aborts through dwt_util_error.
 */
#include "../../include/eaw-experimental.h"
#include "../../include/libdwt.h"
#include "../../include/libdwt_hip.h"

#include <stdlib.h>
#include <string.h>

/* src/libdwt.c:12354 */
void *dwt_util_alloc(int elems, size_t elem_size)
{
	return malloc(elems * elem_size);
}

static int ceil_log2_(int x) /* src/inline.h:443: bits(pow2_ceil_log2(x) - 1), 32 for x == 0 */
{
	int n = 0;
	if (x == 0)
		return 32;
	while (n < 31 && (1 << n) < x)
		n++;
	return n;
}

static int level_limit(int sox, int soy, int decompose_one)
{
	return ceil_log2_(decompose_one ? (sox > soy ? sox : soy) : (sox < soy ? sox : soy));
}

/* a weight buffer of `floats` floats where the image lives */
static float *wbuf_alloc(int dev, long floats, const char *who)
{
	const size_t bytes = (size_t)(floats > 0 ? floats : 1) * sizeof(float);
	float *p = dev ? (float *)dwt_hip_malloc(bytes) : (float *)malloc(bytes);
	if (!p)
		dwt_util_error("%s: cannot allocate %zu bytes of weights\n", who, bytes);
	return p;
}

static void wbuf_free(int dev, float *p)
{
	if (dev)
		dwt_hip_free(p);
	else
		free(p);
}

static void wcopy(int dev, int to_buf, float *buf, float *host, long n, const char *who)
{
	if (n <= 0)
		return;
	if (!dev)
		memcpy(to_buf ? buf : host, to_buf ? host : buf, (size_t)n * sizeof(float));
	else if (to_buf ? dwt_hip_memcpy_h2d(buf, host, (size_t)n * sizeof(float)) : dwt_hip_memcpy_d2h(host, buf, (size_t)n * sizeof(float)))
		dwt_util_error("%s: %s\n", who, dwt_hip_last_error());
}

enum eaw_wavelet { EAW53, EAW97 };

/* the wavelet's device call; 9/7 has the Mallat layout only */
static int eaw_call(enum eaw_wavelet wv, int inverse, int layout, void *ptr, int stride_x, int stride_y, int sox, int soy, int six, int siy,
	int *j, int decompose_one, int zero_padding, float *buf, float alpha)
{
	if (wv == EAW97)
		return dwt_hip_eaw97_2d(inverse, ptr, stride_x, stride_y, sox, soy, six, siy, j, decompose_one, zero_padding, buf, alpha);
	return dwt_hip_eaw53_2d(inverse, layout, ptr, stride_x, stride_y, sox, soy, six, siy, j, decompose_one, zero_padding, buf, alpha);
}

static void eaw_forward(enum eaw_wavelet wv, int layout, void *ptr, int stride_x, int stride_y, int sox, int soy, int six, int siy, int *j_max_ptr,
	int decompose_one, int zero_padding, float *wH[], float *wV[], float alpha, const char *who)
{
	const int lim = level_limit(sox, soy, decompose_one);
	const int J = (*j_max_ptr < 0 || *j_max_ptr > lim) ? lim : *j_max_ptr;
	long off_h[33], off_v[33];
	const long total = dwt_hip_eaw53_weights_layout(layout, sox, soy, six, siy, J, off_h, off_v);
	if (total < 0)
		dwt_util_error("%s: bad sizes\n", who);
	const int dev = dwt_hip_is_device_pointer(ptr);
	float *buf = wbuf_alloc(dev, total, who);
	if (eaw_call(wv, 0, layout, ptr, stride_x, stride_y, sox, soy, six, siy, j_max_ptr, decompose_one, zero_padding, buf, alpha))
		dwt_util_error("%s: %s\n", who, dwt_hip_last_error());
	for (int k = 0; k < J; k++) {
		const long nh = off_v[k] - off_h[k], nv = (k + 1 < J ? off_h[k + 1] : total) - off_v[k];
		wH[k] = dwt_util_alloc((int)nh, sizeof(float));
		wV[k] = dwt_util_alloc((int)nv, sizeof(float));
		wcopy(dev, 0, buf + off_h[k], wH[k], nh, who);
		wcopy(dev, 0, buf + off_v[k], wV[k], nv, who);
	}
	wbuf_free(dev, buf);
}

static void eaw_inverse(enum eaw_wavelet wv, int layout, void *ptr, int stride_x, int stride_y, int sox, int soy, int six, int siy, int j_max,
	int decompose_one, int zero_padding, float *wH[], float *wV[], const char *who)
{
	const int lim = level_limit(sox, soy, decompose_one);
	const int J = (j_max >= 0 && j_max < lim) ? j_max : lim;
	long off_h[33], off_v[33];
	const long total = dwt_hip_eaw53_weights_layout(layout, sox, soy, six, siy, J, off_h, off_v);
	if (total < 0)
		dwt_util_error("%s: bad sizes\n", who);
	const int dev = dwt_hip_is_device_pointer(ptr);
	float *buf = wbuf_alloc(dev, total, who);
	for (int k = 0; k < J; k++) {
		wcopy(dev, 1, buf + off_h[k], wH[k], off_v[k] - off_h[k], who);
		wcopy(dev, 1, buf + off_v[k], wV[k], (k + 1 < J ? off_h[k + 1] : total) - off_v[k], who);
	}
	int j = J;
	if (eaw_call(wv, 1, layout, ptr, stride_x, stride_y, sox, soy, six, siy, &j, decompose_one, zero_padding, buf, 1.f))
		dwt_util_error("%s: %s\n", who, dwt_hip_last_error());
	wbuf_free(dev, buf);
}

/* src/libdwt.c:16663 */
void dwt_eaw53_2f_s(void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int *j_max_ptr, int decompose_one, int zero_padding, float *wH[], float *wV[], float alpha)
{
	eaw_forward(EAW53, DWT_HIP_EAW_MALLAT, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y, j_max_ptr,
		decompose_one, zero_padding, wH, wV, alpha, __func__);
}

/* src/libdwt.c:18373 */
void dwt_eaw53_2i_s(void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int j_max, int decompose_one, int zero_padding, float *wH[], float *wV[])
{
	eaw_inverse(EAW53, DWT_HIP_EAW_MALLAT, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y, j_max,
		decompose_one, zero_padding, wH, wV, __func__);
}

/* src/eaw-experimental.c:300 */
void dwt_eaw97_2f_s(void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int *j_max_ptr, int decompose_one, int zero_padding, float *wH[], float *wV[], float alpha)
{
	eaw_forward(EAW97, DWT_HIP_EAW_MALLAT, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y, j_max_ptr,
		decompose_one, zero_padding, wH, wV, alpha, __func__);
}

/* src/eaw-experimental.c:398 */
void dwt_eaw97_2i_s(void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int j_max, int decompose_one, int zero_padding, float *wH[], float *wV[])
{
	eaw_inverse(EAW97, DWT_HIP_EAW_MALLAT, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y, j_max,
		decompose_one, zero_padding, wH, wV, __func__);
}

/* src/libdwt.c:16602 */
void dwt_eaw53_2f_inplace_s(void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y, int size_i_big_x,
	int size_i_big_y, int *j_max_ptr, int decompose_one, int zero_padding, float *wH[], float *wV[], float alpha)
{
	eaw_forward(EAW53, DWT_HIP_EAW_INTERLEAVED, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y, j_max_ptr,
		decompose_one, zero_padding, wH, wV, alpha, __func__);
}

/* src/libdwt.c:17932 */
void dwt_eaw53_2i_inplace_s(void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y, int size_i_big_x,
	int size_i_big_y, int j_max, int decompose_one, int zero_padding, float *wH[], float *wV[])
{
	eaw_inverse(EAW53, DWT_HIP_EAW_INTERLEAVED, ptr, stride_x, stride_y, size_o_big_x, size_o_big_y, size_i_big_x, size_i_big_y, j_max,
		decompose_one, zero_padding, wH, wV, __func__);
}

/* src/libdwt.c:16759 */
void dwt_eaw53_2f_dummy_s(void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y, int size_i_big_x,
	int size_i_big_y, int *j_max_ptr, int decompose_one)
{
	(void)ptr, (void)stride_x, (void)stride_y, (void)size_i_big_x, (void)size_i_big_y;
	const int lim = level_limit(size_o_big_x, size_o_big_y, decompose_one);
	if (*j_max_ptr < 0 || *j_max_ptr > lim)
		*j_max_ptr = lim;
}
