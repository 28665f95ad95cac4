// dwt_quant.hip -- the deadzone scalar quantizer of ITU-T T.800 Annex E ON THE DEVICE: float coefficient planes (binary32,
// binary16) <-> sign-magnitude indices (int16, int32) with one step per slot of a dense Mallat frame, the per-band
// counters, and the magnitude bit-planes of every code-block.  include/libdwt_hip.h states the arithmetic; DESIGN.md s26
// the kernels.
//
// k_quant.  A lane moves a run of consecutive samples of one row, a wave 64 runs of one row, a workgroup of four waves
// four rows; the run is as long as makes the narrower side one 16-byte access (float <-> int16: 8 samples, two loads and
// one store).  Each side moves by one of two routes, chosen per side on the host (quant_route): wide, 16-byte accesses,
// where the side's base, pitch and batch stride are multiples of 16 bytes; element by element everywhere else and for the
// last, shorter run of a row.  Both routes fill the same registers: same bits.
// The slot of a position follows from the level of its column and the level of its row: the first level at which the
// coordinate falls into the H half (the tables xb / yb of the band geometry), J + 1 for the L half of the last level.
// The row's level is the same for the whole wave; a lane looks up the column level of its run's two ends and takes one
// table entry for the run, or -- where a band boundary lies inside the run -- one per sample.
// No LDS, no scratch, no barrier.  The product |c| * (1 / step) and the sum and product of (|q| + r) * step are rounded
// one by one (no contraction: the Makefile's -ffp-contract=off, repeated below).
//
// k_codeblock_bitplanes.  A wave owns a code-block: its lanes walk the block's rows -- by whole 16-byte chunks where the
// frames' rows are 16-byte aligned, the elements outside the block left out; element by element elsewhere --, reduce the
// largest magnitude across the wave and one lane stores the byte.  The index planes are read once.  (The reading code is
// dwt_codeblock_read.h, shared with the size launch of dwt_bitplane.hip.)
#include "dwt_device.h"
#include "dwt_codeblock_read.h"
#include "dwt_runs.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace dwt {

namespace {

template <int ES>
static __device__ __forceinline__ unsigned elem_load(const char *p)
{
	if constexpr (ES == 2)
		return *(const unsigned short *)p;
	else
		return *(const unsigned *)p;
}
template <int ES>
static __device__ __forceinline__ void elem_store(char *p, unsigned v)
{
	if constexpr (ES == 2)
		*(unsigned short *)p = (unsigned short)v;
	else
		*(unsigned *)p = v;
}

// the level of a coordinate: the smallest j in 1 .. J with x >= bound[j] (bound[] falls with j), J + 1 where there is none
#define QUANT_LEVEL_OF(bound, J, x, out)         \
	do {                                         \
		int l_ = (J) + 1;                        \
		for (int j_ = (J); j_ >= 1; j_--)        \
			l_ = (x) >= (bound)[j_] ? j_ : l_;   \
		(out) = l_;                              \
	} while (0)

// slot 3(j-1) + {0, 1, 2}: HL, LH, HH of level j; 3J: LL of level J
static __device__ __forceinline__ int slot_of(int lx, int ly, int J)
{
	const int j = min(lx, ly);
	return j > J ? 3 * J : 3 * (j - 1) + (lx == j ? (ly == j ? 2 : 0) : 1);
}

static __device__ __forceinline__ void stat_flush(unsigned long long *st, int slot, unsigned nz, unsigned mx, unsigned cl)
{
	unsigned long long *p = st + (long)slot * QUANT_STAT_WORDS;
	if (nz)
		atomicAdd(p, (unsigned long long)nz);
	if (mx)
		atomicMax(p + 1, (unsigned long long)mx);
	if (cl)
		atomicAdd(p + 2, (unsigned long long)cl);
}

template <int COEF, int INDEX, bool INV>
__global__ __launch_bounds__(256) void k_quant(QuantArgs a)
{
	constexpr int CES = quant_coef_es(COEF), IES = quant_index_es(INDEX), RUN = quant_run(COEF, INDEX);
	constexpr float LIM = INDEX == kIndexI16 ? 32768.0f : 2147483648.0f;
	constexpr int TOP = INDEX == kIndexI16 ? 32767 : 2147483647;
	const int wave = threadIdx.x >> 6;
	const long x0 = ((long)blockIdx.x * 64 + (threadIdx.x & 63)) * RUN;
	// (a lane past the row's end stays: the wave reduction of the counters wants all 64)
	const int n = x0 < a.W ? (int)min((long)RUN, a.W - x0) : 0;
	const bool wide_coef = a.wide_coef && n == RUN, wide_index = a.wide_index && n == RUN;
	const int J = a.J, ns = 3 * J + 1;
	int lx_first, lx_last;
	QUANT_LEVEL_OF(a.xb, J, (int)x0, lx_first);
	QUANT_LEVEL_OF(a.xb, J, (int)x0 + n - 1, lx_last);
	const bool one_band = n == 0 || lx_first == lx_last;

	for (int b = blockIdx.z; b < a.batch; b += gridDim.z)
		for (int y = blockIdx.y * QUANT_WG_ROWS + wave; y < a.H; y += gridDim.y * QUANT_WG_ROWS) {
			int ly;
			QUANT_LEVEL_OF(a.yb, J, y, ly);
			const float *const tab = a.tab + (long)b * a.tstride;
			char *const pc = a.coef + (long)b * a.coef_bs + (long)y * a.coef_pitch + x0 * CES;
			char *const pi = a.index + (long)b * a.index_bs + (long)y * a.index_pitch + x0 * IES;
			unsigned cb[RUN], ib[RUN]; // coefficient bits, index bits
			int sl[RUN];               // slots
			float t[RUN];              // the slots' table entries
#pragma unroll
			for (int i = 0; i < RUN; i++)
				cb[i] = ib[i] = 0;

			// ---- the table entries
			if (one_band) {
				const int s = slot_of(lx_first, ly, J);
				const float v = n ? tab[s] : 0.f;
#pragma unroll
				for (int i = 0; i < RUN; i++)
					sl[i] = s, t[i] = v;
			} else {
#pragma unroll
				for (int i = 0; i < RUN; i++) {
					int lx;
					QUANT_LEVEL_OF(a.xb, J, (int)x0 + min(i, n - 1), lx);
					sl[i] = slot_of(lx, ly, J);
					t[i] = tab[sl[i]];
				}
			}

			// ---- load
			if constexpr (!INV) {
				if (wide_coef) {
					run_load<CES>(pc, cb);
				} else {
#pragma unroll
					for (int i = 0; i < RUN; i++)
						if (i < n)
							cb[i] = elem_load<CES>(pc + i * CES);
				}
			} else {
				if (wide_index) {
					run_load<IES>(pi, ib);
				} else {
#pragma unroll
					for (int i = 0; i < RUN; i++)
						if (i < n)
							ib[i] = elem_load<IES>(pi + i * IES);
				}
			}

			// ---- arithmetic (include/libdwt_hip.h)
			unsigned nz = 0, mx = 0, cl = 0; // of the run, where it lies in one band
			unsigned clipped = 0;            // bit i: sample i was clipped
#pragma unroll
			for (int i = 0; i < RUN; i++) {
				if constexpr (!INV) {
					const float c = COEF == kCoefH ? widen_h(cb[i]) : from_bits<float>(cb[i]);
					const bool neg = (cb[i] >> (8 * CES - 1)) & 1;
					const float m = fabsf(c) * t[i];
					const bool in = m < LIM; // (false for NaN)
					const int k = in ? (int)(in ? m : 0.f) : (m != m ? 0 : TOP);
					ib[i] = (unsigned)(neg ? -k : k);
					if (i < n) {
						nz += k != 0;
						mx = max(mx, (unsigned)k);
						cl += !in;
						clipped |= (unsigned)!in << i;
					}
				} else {
					const int q = INDEX == kIndexI16 ? (int)(short)ib[i] : (int)ib[i];
					const unsigned mag = q < 0 ? 0u - (unsigned)q : (unsigned)q;
					float v = ((float)mag + a.r) * t[i];
					v = q < 0 ? -v : v;
					v = q == 0 ? 0.f : v;
					cb[i] = COEF == kCoefH ? narrow_h(v) : to_bits(v);
				}
			}

			// ---- store: the frame's own elements only
			if constexpr (!INV) {
				if (wide_index) {
					run_store<IES>(pi, ib, a.nt_out != 0);
				} else {
#pragma unroll
					for (int i = 0; i < RUN; i++)
						if (i < n)
							elem_store<IES>(pi + i * IES, ib[i]);
				}
			} else {
				if (wide_coef) {
					run_store<CES>(pc, cb, a.nt_out != 0);
				} else {
#pragma unroll
					for (int i = 0; i < RUN; i++)
						if (i < n)
							elem_store<CES>(pc + i * CES, cb[i]);
				}
			}

			// ---- the band counters: integer atomics only, so the sums do not depend on the order
			if constexpr (!INV) {
				if (a.stats) {
					const int copy = (int)((blockIdx.x + blockIdx.y) & (unsigned)(a.stat_copies - 1));
					unsigned long long *const st = a.stats + ((long)copy * a.batch + b) * ns * QUANT_STAT_WORDS;
					const int s_wave = __builtin_amdgcn_readfirstlane(sl[0]); // (lane 0 always holds samples)
					if (__all(n == 0 || (one_band && sl[0] == s_wave))) {
						// the wave lies in one band: one set of atomics for its 64 runs
						unsigned both = nz | cl << 16; // (at most 64 * RUN each)
#pragma unroll
						for (int o = 32; o; o >>= 1) {
							both += __shfl_xor(both, o);
							mx = max(mx, __shfl_xor(mx, o));
						}
						if ((threadIdx.x & 63) == 0)
							stat_flush(st, s_wave, both & 0xffffu, mx, both >> 16);
					} else if (one_band) {
						if (n)
							stat_flush(st, sl[0], nz, mx, cl);
					} else {
						// a band boundary inside the run: sample by sample, one set of atomics per stretch of one slot
						int cur = sl[0];
						unsigned rnz = 0, rmx = 0, rcl = 0;
#pragma unroll
						for (int i = 0; i < RUN; i++)
							if (i < n) {
								if (sl[i] != cur) {
									stat_flush(st, cur, rnz, rmx, rcl);
									cur = sl[i], rnz = rmx = rcl = 0;
								}
								const int q = INDEX == kIndexI16 ? (int)(short)ib[i] : (int)ib[i];
								const unsigned k = (unsigned)(q < 0 ? -q : q);
								rnz += k != 0;
								rmx = max(rmx, k);
								rcl += (clipped >> i) & 1;
							}
						stat_flush(st, cur, rnz, rmx, rcl);
					}
				}
			}
		}
}

template <int INDEX>
__global__ __launch_bounds__(256) void k_codeblock_bitplanes(CodeblockArgs a)
{
	constexpr int ES = quant_index_es(INDEX);
	const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const int per = a.first[a.nslots];
	const long total = (long)a.batch * per;
	for (long g = (long)blockIdx.x * CODEBLOCK_WG_BLOCKS + wave; g < total; g += (long)gridDim.x * CODEBLOCK_WG_BLOCKS) {
		const long b = g / per;
		const int t = (int)(g % per);
		const int k = codeblock_band(a.first, a.nslots, t), ls = t - a.first[k], bx = ls % a.blocks_x[k], by = ls / a.blocks_x[k];
		const int bx0 = bx << a.cbx, by0 = by << a.cby;
		const int cw = min(1 << a.cbx, a.w[k] - bx0), ch = min(1 << a.cby, a.h[k] - by0);
		const char *const p = a.index + b * a.index_bs + (long)(a.y0[k] + by0) * a.index_pitch + (long)(a.x0[k] + bx0) * ES;
		const unsigned mx = codeblock_max_magnitude<INDEX>(p, a.index_pitch, (long)(a.x0[k] + bx0) * ES, cw, ch, a.cbx, a.wide, lane);
		if (lane == 0)
			a.planes[b * a.planes_bs + t] = (unsigned char)(mx ? 32 - __clz(mx) : 0);
	}
}

template <int COEF, int INDEX>
hipError_t quant_go(bool inverse, const QuantArgs &a, dim3 grid, hipStream_t s)
{
	if (inverse)
		k_quant<COEF, INDEX, true><<<grid, 256, 0, s>>>(a);
	else
		k_quant<COEF, INDEX, false><<<grid, 256, 0, s>>>(a);
	return hipGetLastError();
}

} // namespace

hipError_t launch_quant(int coef, int index, bool inverse, const QuantArgs &a, hipStream_t s)
{
	if (a.W < 1 || a.H < 1 || a.batch < 1 || a.J < 0 || a.J > QUANT_MAX_LEVELS || (coef != kCoefS && coef != kCoefH) ||
	    (index != kIndexI16 && index != kIndexI32) || (a.stats && (a.stat_copies < 1 || (a.stat_copies & (a.stat_copies - 1)))))
		return hipErrorInvalidValue;
	// rows and frames past the caps are taken by the kernel's own loops (tests/test_hip_quant.py)
	const long span = 64l * quant_run(coef, index);
	const long gx = (a.W + span - 1) / span, gy = (a.H + QUANT_WG_ROWS - 1) / QUANT_WG_ROWS;
	const dim3 grid((unsigned)gx, (unsigned)std::min<long>(gy, QUANT_GRID_ROWS / QUANT_WG_ROWS), (unsigned)std::min(a.batch, QUANT_GRID_BATCH));
	if (coef == kCoefS)
		return index == kIndexI16 ? quant_go<kCoefS, kIndexI16>(inverse, a, grid, s) : quant_go<kCoefS, kIndexI32>(inverse, a, grid, s);
	return index == kIndexI16 ? quant_go<kCoefH, kIndexI16>(inverse, a, grid, s) : quant_go<kCoefH, kIndexI32>(inverse, a, grid, s);
}

hipError_t launch_codeblock_bitplanes(int index, const CodeblockArgs &a, hipStream_t s)
{
	if (a.nslots < 1 || a.nslots > BAND_MAX_SLOTS || a.batch < 0 || a.cbx < 0 || a.cby < 0 || a.cbx + a.cby > 12 ||
	    (index != kIndexI16 && index != kIndexI32))
		return hipErrorInvalidValue;
	const long total = (long)a.batch * a.first[a.nslots];
	if (total <= 0)
		return hipSuccess;
	// blocks past the cap are taken by the kernel's own loop (tests/test_hip_quant.py)
	const long groups = (total + CODEBLOCK_WG_BLOCKS - 1) / CODEBLOCK_WG_BLOCKS;
	const unsigned grid = (unsigned)std::min<long>(groups, CODEBLOCK_GRID);
	if (index == kIndexI16)
		k_codeblock_bitplanes<kIndexI16><<<grid, 256, 0, s>>>(a);
	else
		k_codeblock_bitplanes<kIndexI32><<<grid, 256, 0, s>>>(a);
	return hipGetLastError();
}

} // namespace dwt
