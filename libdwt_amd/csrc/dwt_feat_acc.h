// dwt_feat_acc.h -- the accumulators and workgroup folds of the feature statistics, shared by the kernels that reduce
// stored coefficients (dwt_features.hip) and the one that reduces coefficients as it computes them (dwt_swt1d.hip): the
// same code, so the same order and the same bits.  Included inside namespace dwt { namespace {.
#pragma once

typedef unsigned long long u64;
// 16 B per lane at any 4-byte alignment: one global_load_dwordx4, which relies on the hardware's unaligned dwordx4 access
// (on by default on gfx9 under ROCm) instead of the row buffers / peeling of dwt_device.h -- no per-row descriptor needed
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));

static __device__ __forceinline__ u64 dbits(double v) { return __builtin_bit_cast(u64, v); }
static __device__ __forceinline__ double bitsd(u64 v) { return __builtin_bit_cast(double, v); }

// order-preserving integer image of a float (negative: all bits flipped, else the sign bit set) and back
static __device__ __forceinline__ unsigned okey(float x)
{
	const unsigned u = to_bits(x);
	return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
static __device__ __forceinline__ float okey_inv(unsigned k) { return from_bits<float>(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

// the float mean as the reference forms it, sum / size with both as floats: the quotient of two floats taken in double
// and rounded to float is the correctly rounded float quotient (53 >= 2*24 + 2)
static __device__ __forceinline__ float mean_of(double s1, long n) { return (float)((double)(float)s1 / (double)(float)(int)n); }

struct Acc1 {
	double s1 = 0, s2 = 0, sp = 0;
	u64 key = 0;
	__device__ __forceinline__ void add(float x, unsigned idx, int pmode, float p)
	{
		const double d = (double)x;
		const float ax = fabsf(x);
		s1 += d;
		s2 += d * d;
		if (pmode == kFeatPAbs)
			sp += (double)ax;
		else if (pmode == kFeatPPow)
			sp += (double)(float)pow((double)ax, (double)p);
		const u64 k = ((u64)to_bits(ax) << 32) | (0xffffffffu - idx);
		key = k > key ? k : key;
	}
};

struct Acc2 {
	double m2 = 0, m3 = 0, m4 = 0;
	__device__ __forceinline__ void add(float x, float c, int mn)
	{
		const float df = x - c;
		const double d = (double)df, d2 = d * d;
		if (mn >= 2 && mn <= 4)
			m2 += d2;
		else // dwt_util_band_moment_s with another exponent: powf(x - c, n)
			m2 += (double)(float)pow(d, (double)mn);
		m3 += d2 * d;
		m4 += d2 * d2;
	}
};

// Sum over the workgroup in a fixed order: lanes by a shuffle tree, then the waves in index order.  Every thread
// returns the total.  sh: NW doubles.
template <int NW>
static __device__ __forceinline__ double wg_sum(double v, double *sh)
{
#pragma unroll
	for (int o = 32; o > 0; o >>= 1)
		v += __shfl_down(v, o);
	if constexpr (NW == 1)
		return __shfl(v, 0);
	if ((threadIdx.x & 63) == 0)
		sh[threadIdx.x >> 6] = v;
	__syncthreads();
	double r = sh[0];
#pragma unroll
	for (int w = 1; w < NW; w++)
		r += sh[w];
	__syncthreads();
	return r;
}

template <int NW>
static __device__ __forceinline__ u64 wg_max(u64 v, u64 *sh)
{
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) {
		const u64 q = __shfl_down(v, o);
		v = q > v ? q : v;
	}
	if constexpr (NW == 1)
		return __shfl(v, 0);
	if ((threadIdx.x & 63) == 0)
		sh[threadIdx.x >> 6] = v;
	__syncthreads();
	u64 r = sh[0];
#pragma unroll
	for (int w = 1; w < NW; w++)
		r = sh[w] > r ? sh[w] : r;
	__syncthreads();
	return r;
}

// The byte of the select that holds rank `k` of a 256-bin histogram: run by one whole wave (lane l takes bins 4l ..
// 4l+3).  Returns the bin to every lane and the rank within it through *k.
static __device__ __forceinline__ unsigned pick_bin(const unsigned *h, unsigned *k)
{
	const int l = threadIdx.x & 63;
	const unsigned b0 = h[4 * l], b1 = h[4 * l + 1], b2 = h[4 * l + 2], b3 = h[4 * l + 3];
	const unsigned mine = b0 + b1 + b2 + b3;
	unsigned inc = mine;
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) {
		const unsigned q = __shfl_up(inc, o);
		if (l >= o)
			inc += q;
	}
	const unsigned exc = inc - mine, kk = *k;
	unsigned bin = 0, rank = 0;
	const bool here = kk >= exc && kk < inc;
	if (here) {
		unsigned r = kk - exc;
		if (r < b0)
			bin = 4 * l;
		else if ((r -= b0) < b1)
			bin = 4 * l + 1;
		else if ((r -= b1) < b2)
			bin = 4 * l + 2;
		else {
			r -= b2;
			bin = 4 * l + 3;
		}
		rank = r;
	}
	// exactly one lane holds it (the ranks asked for lie inside the band)
	const u64 m = __ballot(here);
	const int src = m ? __ffsll((long long)m) - 1 : 0;
	*k = __shfl(rank, src);
	return __shfl(bin, src);
}
