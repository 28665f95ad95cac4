// dwt_band_op.h -- the arithmetic of one band operator on one coefficient, shared by the kernel of the band
// operators (dwt_bandops.hip) and by the inverse stationary transforms, which apply an operator to a detail coefficient
// as they read it (dwt_iswt1d.hip, dwt_iswt2d.hip).  Include inside namespace dwt, in the file's anonymous
// namespace, after dwt_kernels.h (enum BandOp).
#pragma once

// SCALE, HARD and SOFT are float arithmetic as written; COMPRESS, LOG and EXP evaluate pow / log / exp in double and round
// to float once.  A NaN coefficient is left as it is by every operator but ZERO.
template <int OP>
static __device__ __forceinline__ float band_op(float c, float a)
{
	if constexpr (OP == kBandZero)
		return 0.f;
	if (c != c)
		return c;
	if constexpr (OP == kBandScale)
		return c * a;
	if constexpr (OP == kBandHard)
		return fabsf(c) > a ? c : 0.f;
	if constexpr (OP == kBandSoft)
		return c > a ? c - a : (c < -a ? c + a : 0.f);
	if constexpr (OP == kBandCompress) { // hdr.c:101-104: the sign of +0 is -1 there too
		const float s = c > 0.f ? 1.f : -1.f;
		return s * (float)pow((double)fabsf(c), (double)a);
	}
	if constexpr (OP == kMapLog)
		return (float)log((double)(c + a));
	if constexpr (OP == kMapExp)
		return (float)exp((double)c) - a;
	return c;
}

// the operators an inverse stationary transform takes on load (KEEP, ZERO, SCALE, HARD, SOFT), chosen at run time: `op` is
// uniform over a plane, so the branch is too
static __device__ __forceinline__ float band_op_on_load(int op, float c, float a)
{
	switch (op) {
	case kBandZero:
		return 0.f;
	case kBandScale:
		return band_op<kBandScale>(c, a);
	case kBandHard:
		return band_op<kBandHard>(c, a);
	case kBandSoft:
		return band_op<kBandSoft>(c, a);
	default:
		return c;
	}
}
