// dwt_swt_taps.h -- the filters and the tap sums of the stationary wavelet transform, shared by the row kernels
// (dwt_swt1d.hip) and the image kernels (dwt_swt2d.hip).  Include inside namespace dwt, in the file's anonymous namespace.
#pragma once

// The synthesis filters of the inverse are the analysis taps with alternating signs around the centre (exact
// in float): sl[i] = (-1)^(i-CH) * gh[i], the low-pass one of 2*CH+1 taps, and sh[i] = (-1)^(i-CL) * gl[i], the high-pass one.
#define SWT_SYNTHESIS_FILTERS                                                                          \
	static __device__ __forceinline__ float sl(int i) { return ((i - CH) & 1) ? -gh(i) : gh(i); } \
	static __device__ __forceinline__ float sh(int i) { return ((i - CL) & 1) ? -gl(i) : gl(i); }
// the analysis filters as the reference spells them: decimal literals of type double, rounded to float
struct Swt97 {
	static constexpr int CL = 4, CH = 3;
	static __device__ __forceinline__ float gl(int i)
	{
		constexpr float g[9] = {(float)+0.03782846, (float)-0.02384947, (float)-0.11062438, (float)+0.37740287, (float)+0.85269880,
			(float)+0.37740287, (float)-0.11062438, (float)-0.02384947, (float)+0.03782846};
		return g[i];
	}
	static __device__ __forceinline__ float gh(int i)
	{
		constexpr float g[7] = {(float)+0.06453887, (float)-0.04068942, (float)-0.41809219, (float)+0.78848559, (float)-0.41809219,
			(float)-0.04068942, (float)+0.06453887};
		return g[i];
	}
	SWT_SYNTHESIS_FILTERS
};
struct Swt53 {
	static constexpr int CL = 2, CH = 1;
	static __device__ __forceinline__ float gl(int i)
	{
		constexpr float g[5] = {(float)-0.17677669, (float)+0.35355338, (float)+1.06066012, (float)+0.35355338, (float)-0.17677669};
		return g[i];
	}
	static __device__ __forceinline__ float gh(int i)
	{
		constexpr float g[3] = {(float)-0.35355338, (float)+0.70710677, (float)-0.35355338};
		return g[i];
	}
	SWT_SYNTHESIS_FILTERS
};
#undef SWT_SYNTHESIS_FILTERS

// The border rule: the sample that stands for index i outside 0 .. n-1.  SwtClamp replicates the border samples (the
// reference's rule).  SwtReflect is whole-sample symmetric extension, ... x2 x1 | x0 x1 ... : with the symmetric filters of
// odd length every plane of a reflected input is itself symmetric about samples 0 and n-1 at every dilation, so the planes
// extended the same way reconstruct.  Dilations beyond n wrap several times.
struct SwtClamp {
	template <class I>
	static __host__ __device__ __forceinline__ I map(I i, I n)
	{
		i = i < 0 ? 0 : i;
		return i > n - 1 ? n - 1 : i;
	}
};
struct SwtReflect {
	template <class I>
	static __host__ __device__ __forceinline__ I map(I i, I n)
	{
		if (i >= 0 && i < n) // (the interior: no division)
			return i;
		if (n == 1)
			return 0;
		const I P = 2 * (n - 1);
		I m = i % P;
		m = m < 0 ? m + P : m;
		return m > n - 1 ? P - m : m;
	}
};

// Both filters over the 2*CL+1 taps v[k + CL] = x[clamp(p - u*k)], k = -CL .. +CL.  T is float, or a pair of floats that
// are summed side by side (two inputs under the same filter: one packed multiply and one packed add per tap).
template <class F, class T>
static __device__ __forceinline__ void swt_sums(const T *v, T *lo, T *hi)
{
	constexpr int CL = F::CL, CH = F::CH;
	// The sums start from +0.0f and that first addition counts: 0.0f + (-0.0f) is +0.0f.  The compiler drops an addition
	// to a literal zero on this target, so the zero passes through an empty asm and stays a value it cannot see.
	T zero = T(0.0f);
	asm("" : "+v"(zero));
	T l = zero, h = zero;
#pragma unroll
	for (int k = -CL; k <= CL; k++)
		l = l + v[k + CL] * F::gl(k + CL);
#pragma unroll
	for (int k = -CH; k <= CH; k++)
		h = h + v[k + CL] * F::gh(k + CH);
	*lo = l;
	*hi = h;
}

// both outputs at sample p from one read of the taps: x(i) gives input sample i, 0 <= i < n; B is the border rule
template <class F, class I, class B = SwtClamp, class X>
static __device__ __forceinline__ void swt_point(X x, I p, I u, I n, float *lo, float *hi)
{
	constexpr int CL = F::CL;
	float v[2 * CL + 1];
#pragma unroll
	for (int k = -CL; k <= CL; k++)
		v[k + CL] = x(B::map(p - u * k, n));
	swt_sums<F, float>(v, lo, hi);
}

// One inverse step from the taps vl[k + CL] = L[reflect(p - u*k)] (used for |k| <= CH) and vh[k + CL] = H[reflect(p - u*k)]:
// 0.5f * (conv(L, sl) + conv(H, sh)), each sum from +0.0f as in swt_sums, every product and sum rounded on its own.
template <class F, class T>
static __device__ __forceinline__ T iswt_sums(const T *vl, const T *vh)
{
	constexpr int CL = F::CL, CH = F::CH;
	T zero = T(0.0f);
	asm("" : "+v"(zero));
	T l = zero, h = zero;
#pragma unroll
	for (int k = -CH; k <= CH; k++)
		l = l + vl[k + CL] * F::sl(k + CH);
#pragma unroll
	for (int k = -CL; k <= CL; k++)
		h = h + vh[k + CL] * F::sh(k + CL);
	return (l + h) * 0.5f;
}

// the inverse at sample p: xl(i) and xh(i) give sample i of the level's L and H plane, 0 <= i < n
template <class F, class I, class XL, class XH>
static __device__ __forceinline__ float iswt_point(XL xl, XH xh, I p, I u, I n)
{
	constexpr int CL = F::CL, CH = F::CH;
	float vl[2 * CL + 1], vh[2 * CL + 1];
#pragma unroll
	for (int k = -CL; k <= CL; k++) {
		const I i = SwtReflect::map(p - u * k, n);
		vh[k + CL] = xh(i);
		vl[k + CL] = (k >= -CH && k <= CH) ? xl(i) : 0.f;
	}
	return iswt_sums<F, float>(vl, vh);
}
