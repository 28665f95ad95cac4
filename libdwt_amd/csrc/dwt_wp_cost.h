// dwt_wp_cost.h -- one coefficient's term of an additive best-basis cost (enum dwt_hip_wp_cost), shared
// by the line kernels (dwt_wp_basis.hip) and the image kernels (dwt_wp_basis2d.hip).
#pragma once
#include "dwt_kernels.h"

#include <cfloat>
#include <cmath>

namespace dwt {

// a non-finite coefficient gives NaN
static __device__ __forceinline__ double wp_term(int kind, float param, float c)
{
	if (!(fabsf(c) <= FLT_MAX))
		return (double)NAN;
	const double x = (double)c, e = x * x;
	switch (kind) {
	case kWpCostShannon: return e == 0 ? 0.0 : -e * log(e);
	case kWpCostLogEnergy: return e == 0 ? 0.0 : log(e);
	case kWpCostLp: return param == 1.0f ? fabs(x) : pow(fabs(x), (double)param);
	default: return fabsf(c) > param ? 1.0 : 0.0;
	}
}

} // namespace dwt
