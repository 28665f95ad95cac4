// dwt_swt_taps.h -- the filters and the tap sums of the stationary wavelet transform, shared by the row kernels
// (dwt_swt1d.hip) and the image kernels (dwt_swt2d.hip).  Include inside namespace dwt, in the file's anonymous namespace.
#pragma once

// the filters as the reference spells them: decimal literals of type double, rounded to float
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

// both outputs at sample p from one read of the taps: x(i) gives input sample i, 0 <= i < n
template <class F, class I, class X>
static __device__ __forceinline__ void swt_point(X x, I p, I u, I n, float *lo, float *hi)
{
	constexpr int CL = F::CL;
	float v[2 * CL + 1];
#pragma unroll
	for (int k = -CL; k <= CL; k++) {
		I i = p - u * k;
		i = i < 0 ? 0 : i;
		i = i > n - 1 ? n - 1 : i;
		v[k + CL] = x(i);
	}
	swt_sums<F, float>(v, lo, hi);
}
