/*
 * dwt_entry_timefreq.c -- the host side of the time-frequency entries (include/gabor.h, include/libdwt_hip.h; DESIGN.md
 * s14): the kernel generators of the STFT, the CWT and the S transform, and dwt_util_cdot1_s.
 *
 * The generators restate the reference's expressions (src/gabor.c) operation by operation in float, through the host's
 * libm as the reference does, so a bank generated here holds the taps the reference would correlate with:
 *   atom(t, alpha, omega) = sqrtf(alpha / pi) * expf(-alpha * t * t) * cexpf(i * omega * t)
 *   wavelet(t, sigma, f, a) = 1 / |a| * atom(t / a, 1 / 2 / sigma / sigma, f)
 *   size(sigma, a) = (int)ceilf(1 + 2 * ((4 * sigma) * a)),  centre = size / 2
 * dwt_util_cdot1_s logs the reason and aborts through dwt_util_error where it cannot run on the device, as the other
 * entries of libdwt do.
 */
#include "../../include/libdwt.h"
#include "../../include/libdwt_hip.h"
#include "../../include/gabor.h"

#include <complex.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

static float complex atom(float t, float alpha, float omega)
{
	return sqrtf(alpha / (float)M_PI) * expf(-alpha * t * t) * cexpf(+I * omega * t);
}

static float complex wavelet(float t, float sigma, float f, float a)
{
	const float alpha = 1.f / 2.f / sigma / sigma;
	t /= a;
	return 1.f / fabsf(a) * atom(t, alpha, f);
}

static float size_f(float sigma, float a)
{
	return ceilf(1.f + 2.f * ((4.f * sigma) * a));
}

int dwt_hip_gaussian_size(float sigma, float a)
{
	return (int)size_f(sigma, a);
}

void dwt_hip_gabor_wavelet(float t, float sigma, float f, float a, float *re_im)
{
	const float complex z = wavelet(t, sigma, f, a);
	re_im[0] = crealf(z);
	re_im[1] = cimagf(z);
}

/* the S transform's kernel of frequency f (cycles per sample): a Gaussian of alpha = f * f around integer t */
static float s_sigma(float f)
{
	return sqrtf(1.f / 2.f / (f * f));
}

static void put(void *kern, int stride, int i, float complex z)
{
	const float v[2] = {crealf(z), cimagf(z)};
	memcpy((char *)kern + (size_t)i * stride, v, sizeof v);
}

void dwt_hip_gabor_gen_kernel(void *kern, int stride, float sigma, float freq, float a)
{
	const int size = dwt_hip_gaussian_size(sigma, a), center = size / 2;
	for (int i = 0; i < size; i++)
		put(kern, stride, i, wavelet(i - center, sigma, freq, a));
}

static void s_gen_kernel(void *kern, int stride, float f)
{
	const float alpha = f * f, omega = 2.f * (float)M_PI * f;
	const int size = dwt_hip_gaussian_size(s_sigma(f), 1.f), center = size / 2;
	for (int i = 0; i < size; i++) {
		const int t = i - center;
		put(kern, stride, i, atom(t, alpha, omega));
	}
}

/* bin y of a transform of `bins` bins: the scale and the Gaussian's width that fix its size; WT and ST also the frequency */
static void bin_params(int kind, int y, int bins, float sigma, float freq, float *f, float *a, float *sig)
{
	const float norm1 = (y + 1.f) / (float)bins;
	*a = 1.f;
	*sig = sigma;
	if (kind == DWT_HIP_TIMEFREQ_FT)
		*f = (y / (float)bins) * 1.0f * (float)M_PI;
	else if (kind == DWT_HIP_TIMEFREQ_WT) {
		*f = norm1 * 0.5f * 2.f * (float)M_PI;
		*a = freq / *f;
	} else {
		*f = norm1 * 0.5f;
		*sig = s_sigma(*f);
	}
}

/* The kernels of a whole transform, for dwt_hip_timefreq_bank_create (dwt_backend_timefreq.hip): sizes[bins] and
 * centers[bins] are always written; taps, unless NULL, takes every kernel's (re, im) pairs one after the other.  Returns
 * the number of taps of all kernels together, or -1 where a size is not a number an int holds. */
__attribute__((visibility("hidden"))) long dwt_tf_generate(int kind, int bins, float sigma, float freq, int *sizes, int *centers, float *taps)
{
	long total = 0;
	for (int y = 0; y < bins; y++) {
		float f, a, sig;
		bin_params(kind, y, bins, sigma, freq, &f, &a, &sig);
		const float s = size_f(sig, a);
		if (!(s >= 1.f && s < 1e9f)) /* (also NaN) */
			return -1;
		sizes[y] = (int)s;
		centers[y] = sizes[y] / 2;
		if (taps) {
			if (kind == DWT_HIP_TIMEFREQ_ST)
				s_gen_kernel(taps + 2 * total, 8, f);
			else
				dwt_hip_gabor_gen_kernel(taps + 2 * total, 8, sigma, kind == DWT_HIP_TIMEFREQ_FT ? f : freq, a);
		}
		total += sizes[y];
	}
	return total;
}

float complex dwt_util_cdot1_s(const float *func, int func_size, int func_stride, int func_center, const float complex *kern, int kern_size,
	int kern_stride, int kern_center)
{
	float v[2] = {0.f, 0.f};
	if (dwt_hip_cdot1(func, func_size, func_stride, func_center, (const float *)kern, kern_size, kern_stride, kern_center, v))
		dwt_util_error("%s: %s\n", __func__, dwt_hip_last_error());
	float complex z;
	memcpy(&z, v, sizeof z);
	return z;
}
