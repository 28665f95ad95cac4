// dwt_nterm.hip -- the kernels of the N-term approximation: what the non-linear branch of the
// reference's examples/displ-vectors/vectors.c (:254-297) does between its forward and its inverse transforms -- the
// magnitude of every position over the transforms of 1 .. 4 channels, the magnitude of descending rank N as threshold,
// +0 into every channel of every position below it -- on coefficients that stay where they lie.
//
// Magnitude, in float, every product and sum rounded on its own, left to right, the root correctly rounded:
// fabsf(c0) for one channel, sqrtf(c0*c0 + c1*c1 [+ c2*c2 [+ c3*c3]]) otherwise.  It is never negative and never -0,
// so its uint32 image (the KEY) orders as the float does.  The key is recomputed from the coefficients by every pass;
// no magnitude plane exists outside dwt_hip_magnitude_batch.
//
// A radix select over the key's 31 bits, 11 + 10 + 10 from the top: histogram launch p counts digit p of the keys
// whose higher digits equal the ones already chosen, into a workgroup histogram in LDS that is flushed with one global
// integer atomic per non-empty bin.  No launch picks a digit: every workgroup of the NEXT launch reads the small global
// histogram of the one before, finds the bin that holds the rank and the rank left inside it (narrow), and the first
// workgroup of a group records that for the launch after.  The apply launch narrows the last time -- the three digits
// are the threshold's key, the keys above it are the rank asked for less the rank left, the last bin's count the ties --
// and zeroes.  Integer atomics commute: a call gives the same bits on every run and for every grid.
//
// One launch walks every group: workgroup i takes slabs i % bpg, i % bpg + bpg, .. of group i / bpg, a slab being
// slab_rows rows; a power of two of lanes lies along a row, each on 4 adjacent positions of every channel (one 16-byte
// access per channel where every base and stride allows it and the quad lies inside the row, single elements otherwise),
// the other lanes on further rows.  Nothing outside a row's own elements is read or written, nothing outside the scope
// decides or is written.
#include "dwt_device.h"
#include "dwt_kernels.h"

namespace dwt {

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

enum { kHist0 = 0, kHist1, kHist2, kApply, kMagnitude };

template <int C>
static __device__ __forceinline__ float magnitude(const float (&c)[NTERM_MAX_CH][4], int e)
{
	if constexpr (C == 1)
		return fabsf(c[0][e]); // (exact; sqrtf(c*c) would lose every |c| below 2^-75)
	float s = c[0][e] * c[0][e] + c[1][e] * c[1][e];
	if constexpr (C >= 3)
		s = s + c[2][e] * c[2][e];
	if constexpr (C >= 4)
		s = s + c[3][e] * c[3][e];
	return sqrtf(s);
}

// The bin that holds the element of descending rank `rank` (1-based) of a histogram of 256 * CN counters -> bin, the
// rank left inside that bin -> rank, the bin's count -> cnt.  All 256 threads; sh: 8 words of LDS.
template <int CN>
static __device__ __forceinline__ void narrow(const unsigned *h, unsigned &rank, unsigned &bin, unsigned &cnt, unsigned *sh)
{
	const int t = threadIdx.x, top = 256 * CN - 1 - t * CN; // thread t: bins top, top - 1, .. top - CN + 1
	unsigned v[CN], s = 0;
#pragma unroll
	for (int i = 0; i < CN; i++) {
		v[i] = h[top - i];
		s += v[i];
	}
	unsigned inc = s;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const unsigned o = __shfl_up(inc, d);
		if ((t & 63) >= d)
			inc += o;
	}
	if ((t & 63) == 63)
		sh[t >> 6] = inc;
	if (t == 0)
		sh[4] = sh[5] = sh[6] = 0;
	__syncthreads();
	unsigned excl = inc - s;
	for (int w = 0; w < (t >> 6); w++)
		excl += sh[w];
	if (excl < rank && rank <= excl + s) { // one thread at most
		unsigned r = rank - excl;
		bool done = false;
#pragma unroll
		for (int i = 0; i < CN; i++)
			if (!done) {
				if (v[i] >= r) {
					sh[4] = (unsigned)(top - i);
					sh[5] = r;
					sh[6] = v[i];
					done = true;
				} else
					r -= v[i];
			}
	}
	__syncthreads();
	bin = sh[4];
	rank = sh[5];
	cnt = sh[6];
	__syncthreads();
}

template <int C, int MODE>
__global__ __launch_bounds__(256) void k_nterm(NtermArgs a)
{
	constexpr int NB = MODE == kHist0 ? NTERM_BINS0 : (MODE == kHist1 ? NTERM_BINS1 : (MODE == kHist2 ? NTERM_BINS2 : 1));
	constexpr bool kHist = MODE <= kHist2;
	__shared__ unsigned hist[NB];
	__shared__ unsigned sh[8];
	const int g = blockIdx.x / a.bpg, b0 = blockIdx.x % a.bpg;
	unsigned *gh = a.hist + (long)g * NTERM_HIST, *rec = a.rec + (long)g * NTERM_REC;

	// what the launches before this one have chosen
	unsigned prefix = 0;
	if constexpr (MODE == kHist1 || MODE == kHist2 || MODE == kApply) {
		unsigned rank = a.rank[g], bin, cnt;
		if constexpr (MODE == kHist1) {
			narrow<NTERM_BINS0 / 256>(gh, rank, bin, cnt, sh);
			prefix = bin;
		} else {
			prefix = rec[MODE == kHist2 ? 0 : 2];
			rank = rec[MODE == kHist2 ? 1 : 3];
			narrow<NTERM_BINS1 / 256>(gh + (MODE == kHist2 ? NTERM_BINS0 : NTERM_BINS0 + NTERM_BINS1), rank, bin, cnt, sh);
			prefix = prefix << 10 | bin;
		}
		if (b0 == 0 && threadIdx.x == 0) {
			if constexpr (MODE == kApply) {
				rec[4] = prefix;                       // the threshold's key
				rec[5] = a.rank[g] - rank + cnt;       // keys above it, and its ties
			} else {
				rec[MODE == kHist1 ? 0 : 2] = prefix;
				rec[MODE == kHist1 ? 1 : 3] = rank;
			}
		}
	}
	if constexpr (kHist) {
		for (int i = threadIdx.x; i < NB; i += 256)
			hist[i] = 0;
		__syncthreads();
	}

	const int q = (a.w + 3) >> 2;
	int lg = 0;
	while (lg < 8 && (1 << lg) < q)
		lg++;
	const int TX = 1 << lg, TY = 256 >> lg, tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> lg;
	char *base = a.img + (long)g * a.bstride;
	for (int slab = b0; slab < a.slabs; slab += a.bpg) { // (past the cap: tests/test_hip_grid_limits.py)
		const int r0 = slab * a.slab_rows, rows = min(a.slab_rows, a.h - r0);
		for (int r = ty; r < rows; r += TY) {
			const int y = r0 + r;
			char *row = base + (long)y * a.pitch;
			for (int i = tx; i < q; i += TX) {
				const int x = 4 * i, nv = min(4, a.w - x);
				const bool quad = a.vec && nv == 4;
				float c[NTERM_MAX_CH][4];
#pragma unroll
				for (int k = 0; k < C; k++) {
					const float *p = (const float *)(row + k * a.cstride) + x;
					if (quad) {
						const f4 v = *(const f4 *)p;
						c[k][0] = v.x;
						c[k][1] = v.y;
						c[k][2] = v.z;
						c[k][3] = v.w;
					} else {
#pragma unroll
						for (int e = 0; e < 4; e++)
							c[k][e] = e < nv ? p[e] : 0.f;
					}
				}
				float m[4];
				bool in[4], zero[4];
				bool all_in = true, any_zero = false;
#pragma unroll
				for (int e = 0; e < 4; e++) {
					m[e] = magnitude<C>(c, e);
					in[e] = e < nv && (MODE == kMagnitude || !(x + e < a.lx && y < a.ly));
					all_in = all_in && in[e];
					const unsigned key = __float_as_uint(m[e]) & 0x7fffffffu;
					if constexpr (MODE == kHist0) {
						if (in[e])
							atomicAdd(&hist[key >> 20], 1u);
					} else if constexpr (MODE == kHist1) {
						if (in[e] && key >> 20 == prefix)
							atomicAdd(&hist[key >> 10 & 1023u], 1u);
					} else if constexpr (MODE == kHist2) {
						if (in[e] && key >> 10 == prefix)
							atomicAdd(&hist[key & 1023u], 1u);
					} else if constexpr (MODE == kApply) {
						zero[e] = in[e] && key < prefix;
						any_zero = any_zero || zero[e];
					}
				}
				if constexpr (MODE == kApply) {
					if (!any_zero)
						continue;
#pragma unroll
					for (int k = 0; k < C; k++) {
						float *p = (float *)(row + k * a.cstride) + x;
						if (quad && all_in) {
							*(f4 *)p = f4{zero[0] ? 0.f : c[k][0], zero[1] ? 0.f : c[k][1], zero[2] ? 0.f : c[k][2], zero[3] ? 0.f : c[k][3]};
						} else {
#pragma unroll
							for (int e = 0; e < 4; e++)
								if (zero[e])
									p[e] = 0.f;
						}
					}
				}
				if constexpr (MODE == kMagnitude) {
					float *p = (float *)(a.map + (long)g * a.map_bstride + (long)y * a.map_pitch) + x;
					if (quad) {
						*(f4 *)p = f4{m[0], m[1], m[2], m[3]};
					} else {
#pragma unroll
						for (int e = 0; e < 4; e++)
							if (e < nv)
								p[e] = m[e];
					}
				}
			}
		}
	}

	if constexpr (kHist) {
		__syncthreads();
		unsigned *out = gh + (MODE == kHist0 ? 0 : (MODE == kHist1 ? NTERM_BINS0 : NTERM_BINS0 + NTERM_BINS1));
		for (int i = threadIdx.x; i < NB; i += 256) {
			const unsigned n = hist[i];
			if (n)
				atomicAdd(&out[i], n);
		}
	}
}

template <int MODE>
hipError_t launch(const NtermArgs &a, hipStream_t s)
{
	if (a.channels < 1 || a.channels > NTERM_MAX_CH || a.batch < 0 || a.w < 0 || a.h < 0 || a.bpg < 1 || a.slab_rows < 1 || a.slabs < 0)
		return hipErrorInvalidValue;
	const long grid = (long)a.batch * a.bpg;
	if (grid <= 0 || a.slabs == 0 || a.w == 0)
		return hipSuccess;
	if (grid > 0x7fffffffl || (long)(a.slabs - 1) * a.slab_rows >= a.h || (long)a.slabs * a.slab_rows < a.h)
		return hipErrorInvalidValue;
	switch (a.channels) {
	case 1:
		k_nterm<1, MODE><<<(unsigned)grid, 256, 0, s>>>(a);
		break;
	case 2:
		k_nterm<2, MODE><<<(unsigned)grid, 256, 0, s>>>(a);
		break;
	case 3:
		k_nterm<3, MODE><<<(unsigned)grid, 256, 0, s>>>(a);
		break;
	default:
		k_nterm<4, MODE><<<(unsigned)grid, 256, 0, s>>>(a);
		break;
	}
	return hipGetLastError();
}

} // namespace

hipError_t launch_nterm_hist(const NtermArgs &a, int pass, hipStream_t s)
{
	if (!a.rank || !a.hist || !a.rec)
		return hipErrorInvalidValue;
	switch (pass) {
	case 0:
		return launch<kHist0>(a, s);
	case 1:
		return launch<kHist1>(a, s);
	case 2:
		return launch<kHist2>(a, s);
	}
	return hipErrorInvalidValue;
}

hipError_t launch_nterm_apply(const NtermArgs &a, hipStream_t s)
{
	if (!a.rank || !a.hist || !a.rec)
		return hipErrorInvalidValue;
	return launch<kApply>(a, s);
}

hipError_t launch_nterm_magnitude(const NtermArgs &a, hipStream_t s)
{
	if (!a.map)
		return hipErrorInvalidValue;
	return launch<kMagnitude>(a, s);
}

} // namespace dwt
