// dwt_feat_acc.h -- the accumulators and workgroup folds of the feature statistics and the reduction of one record over
// them (reduce_record), shared by the kernel that reduces stored lines (k_feat_lines, dwt_features.hip) and the one that
// reduces coefficients as it computes them (k_swt_lines, dwt_swt1d.hip): the same code, so the same order and the same
// bits.  Included inside namespace dwt { namespace {.
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

// The `n` values of one record -> its raw planes rec[plane * nrec + r], by the NT threads of one line (this one is t;
// NT = 64: one wave of a shared workgroup, else the whole workgroup).  first(i) gives value i in the pass every call
// makes (k_swt_lines computes the sample there and keeps its low-pass part), again(i) gives it to the passes that read
// the values once more: the central moments about the float mean (work & kFeatPass2) and the four rounds of the median's
// radix select (work & kFeatSelect).  Thread t takes values t, t + NT, ...; every thread of the workgroup meets every
// barrier, a thread that is not `active` stores nothing.  shd, shk: 4 entries each; hist: 256; sel: 2.
template <int NT, class First, class Again>
static __device__ __forceinline__ void reduce_record(int t, int n, First first, Again again, long r, u64 *rec, long nrec, int work,
	int pmode, float p, bool active, double *shd, u64 *shk, unsigned *hist, unsigned *sel)
{
	constexpr int NW = NT / 64;
	Acc1 acc;
	for (int i = t; i < n; i += NT)
		acc.add(first(i), (unsigned)i, pmode, p);
	const double s1 = wg_sum<NW>(acc.s1, shd), s2 = wg_sum<NW>(acc.s2, shd);
	const double sp = pmode != kFeatPNone ? wg_sum<NW>(acc.sp, shd) : 0.0;
	const u64 key = wg_max<NW>(acc.key, shk);
	if (t == 0 && active) {
		rec[kFeatS1 * nrec + r] = dbits(s1);
		rec[kFeatS2 * nrec + r] = dbits(s2);
		rec[kFeatSp * nrec + r] = dbits(sp);
		rec[kFeatKey * nrec + r] = key;
	}
	if (work & kFeatPass2) {
		const float c = mean_of(s1, n);
		Acc2 m;
		for (int i = t; i < n; i += NT)
			m.add(again(i), c, 2);
		const double m2 = wg_sum<NW>(m.m2, shd), m3 = wg_sum<NW>(m.m3, shd), m4 = wg_sum<NW>(m.m4, shd);
		if (t == 0 && active) {
			rec[kFeatM2 * nrec + r] = dbits(m2);
			rec[kFeatM3 * nrec + r] = dbits(m3);
			rec[kFeatM4 * nrec + r] = dbits(m4);
		}
	}
	if (work & kFeatSelect) {
		unsigned prefix = 0, rank = (unsigned)n / 2;
		for (int pass = 0; pass < 4; pass++) {
			const int shift = 24 - 8 * pass;
			for (int i = t; i < 256; i += NT)
				hist[i] = 0;
			__syncthreads();
			for (int i = t; i < n; i += NT) {
				const unsigned q = okey(again(i));
				if (pass == 0 || (q >> (shift + 8)) == prefix)
					atomicAdd(&hist[(q >> shift) & 255], 1u);
			}
			__syncthreads();
			if (t < 64) {
				unsigned kk = rank;
				const unsigned bin = pick_bin(hist, &kk);
				if (t == 0) {
					sel[0] = bin;
					sel[1] = kk;
				}
			}
			__syncthreads();
			prefix = (prefix << 8) | sel[0];
			rank = sel[1];
			__syncthreads();
		}
		if (t == 0 && active)
			rec[kFeatMed * nrec + r] = to_bits(okey_inv(prefix));
	}
}
