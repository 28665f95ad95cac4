// dwt_bitplane.hip -- embedded bit-plane streams of code-blocks ON THE DEVICE: every code-block of an int16 / int32 index
// frame as a sign plane and its magnitude planes, most significant first, in 64-bit words of 64 samples, the blocks in
// stream order; and back, with the least significant planes left out on request.  include/libdwt_hip.h states the format;
// DESIGN.md s36 the kernels.
//   k_bitplane_sizes        launch 1: a wave owns a block, reads its largest magnitude (dwt_codeblock_read.h, the reading code
//                           of k_codeblock_bitplanes with its 16-byte route) and stores the block's size in words.
//   k_bitplane_scan         launch 2: one workgroup per frame turns the sizes into the frame's offsets.
//   k_bitplane_pack         launch 3: a workgroup owns a block.  p follows from the offsets.  A wave takes groups of 64
//                           samples, lane i sample 64 g + i; a plane's word is one 64-bit ballot.  The block's words are
//                           assembled in LDS and leave as one contiguous run, 16-byte stores where the run's base allows.
//   k_bitplane_unpack       the way back: the planes that are read go contiguously into LDS, a lane gathers its bit of
//                           every plane word (the wave reads one word: a broadcast) and writes its element, zeros included;
//                           where the block's rows start on 16-byte boundaries a lane gathers a run of 16 bytes instead and
//                           stores it by one access.
//   k_bitplane_pack_plain, k_bitplane_unpack_plain   the cross-check route (option "bitplane_wave" = 0): one lane builds or
//                           consumes one word by touching its 64 samples itself; no ballots, no LDS.  Same bytes.
// The order is fixed by construction: no atomics, no workgroup waits for another.  No arithmetic on the values.
#include "dwt_codeblock_read.h"
#include "dwt_device.h"

#include <algorithm>

namespace dwt {

namespace {

typedef unsigned long long u64;
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

// the rectangle of block t of a frame: band k (stream order), its first sample in frame coordinates, its width and height
struct BlockRect {
	int x, y, cw, ch;
};
static __device__ __forceinline__ BlockRect block_rect(const BitplaneArgs &a, int t)
{
	const int k = codeblock_band(a.first, a.bands, t), ls = t - a.first[k], bx = ls % a.blocks_x[k], by = ls / a.blocks_x[k];
	const int bx0 = bx << a.cbx, by0 = by << a.cby;
	return BlockRect{a.x0[k] + bx0, a.y0[k] + by0, min(1 << a.cbx, a.w[k] - bx0), min(1 << a.cby, a.h[k] - by0)};
}

template <int ES>
static __device__ __forceinline__ int index_load(const char *p)
{
	if constexpr (ES == 2)
		return (int)__builtin_nontemporal_load((const short *)p);
	else
		return __builtin_nontemporal_load((const int *)p);
}
template <int ES>
static __device__ __forceinline__ void index_store(char *p, unsigned v, bool nt)
{
	if constexpr (ES == 2) {
		if (nt)
			__builtin_nontemporal_store((unsigned short)v, (unsigned short *)p);
		else
			*(unsigned short *)p = (unsigned short)v;
	} else {
		if (nt)
			__builtin_nontemporal_store(v, (unsigned *)p);
		else
			*(unsigned *)p = v;
	}
}
static __device__ __forceinline__ unsigned magnitude(int q) { return q < 0 ? 0u - (unsigned)q : (unsigned)q; }

template <int INDEX>
__global__ __launch_bounds__(256) void k_bitplane_sizes(BitplaneArgs a)
{
	constexpr int ES = quant_index_es(INDEX);
	const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const long total = (long)a.batch * a.blocks;
	for (long g = (long)blockIdx.x * BITPLANE_WG_BLOCKS + wave; g < total; g += (long)gridDim.x * BITPLANE_WG_BLOCKS) {
		const long b = g / a.blocks;
		const int t = (int)(g % a.blocks);
		const BlockRect r = block_rect(a, t);
		const char *const p = a.index + b * a.bs + (long)r.y * a.pitch + (long)r.x * ES;
		const unsigned mx = codeblock_max_magnitude<INDEX>(p, a.pitch, (long)r.x * ES, r.cw, r.ch, a.cbx, a.wide, lane);
		if (lane == 0) {
			const unsigned planes = mx ? 32 - __clz(mx) : 0, groups = (unsigned)(r.cw * r.ch + 63) >> 6;
			a.sizes[g] = planes ? (planes + 1) * groups : 0u;
		}
	}
}

constexpr int SCAN_ITEMS = 8; // consecutive blocks of a thread per trip

__global__ __launch_bounds__(256) void k_bitplane_scan(BitplaneArgs a)
{
	__shared__ unsigned wsum[4];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for (int b = blockIdx.x; b < a.batch; b += gridDim.x) {
		const unsigned *const sz = a.sizes + (long)b * a.blocks;
		unsigned *const off = a.offsets + (long)b * (a.blocks + 1);
		unsigned carry = 0;
		for (int t0 = 0; t0 < a.blocks; t0 += 256 * SCAN_ITEMS) {
			const int i0 = t0 + (int)threadIdx.x * SCAN_ITEMS;
			unsigned c[SCAN_ITEMS], sum = 0;
#pragma unroll
			for (int i = 0; i < SCAN_ITEMS; i++) {
				c[i] = i0 + i < a.blocks ? sz[i0 + i] : 0u;
				sum += c[i];
			}
			unsigned incl = sum; // inclusive over the wave's lanes
#pragma unroll
			for (int o = 1; o < 64; o <<= 1) {
				const unsigned up = __shfl_up(incl, o);
				incl += lane >= o ? up : 0u;
			}
			if (lane == 63)
				wsum[wave] = incl;
			__syncthreads();
			unsigned below = 0, all = 0;
#pragma unroll
			for (int q = 0; q < 4; q++) {
				below += q < wave ? wsum[q] : 0u;
				all += wsum[q];
			}
			unsigned at = carry + below + incl - sum;
#pragma unroll
			for (int i = 0; i < SCAN_ITEMS; i++)
				if (i0 + i < a.blocks) {
					off[i0 + i] = at;
					at += c[i];
				}
			carry += all;
			__syncthreads(); // (wsum is written again)
		}
		if (threadIdx.x == 0)
			off[a.blocks] = carry;
	}
}

constexpr int PACK_TRIP = 8; // groups of a wave whose loads are in flight together

template <int INDEX>
__global__ __launch_bounds__(256) void k_bitplane_pack(BitplaneArgs a)
{
	constexpr int ES = quant_index_es(INDEX);
	__shared__ u64 lds[BITPLANE_MAX_WORDS];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const long total = (long)a.batch * a.blocks;
	for (long gb = blockIdx.x; gb < total; gb += gridDim.x) {
		const long b = gb / a.blocks;
		const int t = (int)(gb % a.blocks);
		const unsigned *const off = a.offsets + b * (a.blocks + 1);
		const unsigned o0 = off[t], o1 = off[t + 1];
		if (o1 == o0 || o1 > a.stream_stride)
			continue; // (the whole workgroup: a block of zeros, or one past the capacity)
		const BlockRect r = block_rect(a, t);
		const int n = r.cw * r.ch, G = (n + 63) >> 6, nw = (int)(o1 - o0), p = nw / G - 1;
		const bool full = r.cw == (1 << a.cbx);
		const char *const src = a.index + b * a.bs + (long)r.y * a.pitch + (long)r.x * ES;
		// a wave takes PACK_TRIP consecutive groups a trip: their loads are in flight together, then the ballots
		for (int g0 = wave * PACK_TRIP; g0 < G; g0 += 4 * PACK_TRIP) {
			int q[PACK_TRIP];
#pragma unroll
			for (int u = 0; u < PACK_TRIP; u++) {
				const int i = 64 * (g0 + u) + lane;
				q[u] = 0;
				if (i < n) { // (a group past the block's last holds no sample)
					const int y = full ? i >> a.cbx : i / r.cw, x = i - y * r.cw;
					q[u] = index_load<ES>(src + (long)y * a.pitch + (long)x * ES);
				}
			}
#pragma unroll
			for (int u = 0; u < PACK_TRIP; u++) {
				if (g0 + u >= G)
					break; // (the whole wave)
				const unsigned mag = magnitude(q[u]);
				u64 mine = __ballot(q[u] < 0); // lane k keeps plane k's word
				for (int k = 1; k <= p; k++) {
					const u64 m = __ballot((mag >> (p - k)) & 1u);
					mine = lane == k ? m : mine;
				}
				if (lane <= p)
					lds[lane * G + g0 + u] = mine;
			}
		}
		__syncthreads();
		// the block's words leave as one run: a word in front where the run starts on an odd word, then pairs
		u64 *const dst = a.words + (u64)b * a.stream_stride + o0;
		const int head = (int)(((uintptr_t)dst >> 3) & 1), pairs = (nw - head) >> 1;
		for (int i = threadIdx.x; i < pairs; i += 256) {
			const u64x2 v = {lds[head + 2 * i], lds[head + 2 * i + 1]};
			*(u64x2 *)(dst + head + 2 * i) = v;
		}
		if (threadIdx.x == 0 && head)
			dst[0] = lds[0];
		if (threadIdx.x == 64 && ((nw - head) & 1))
			dst[nw - 1] = lds[nw - 1];
		__syncthreads(); // (the next block's words go into the same LDS)
	}
}

template <int INDEX>
__global__ __launch_bounds__(256) void k_bitplane_pack_plain(BitplaneArgs a)
{
	constexpr int ES = quant_index_es(INDEX);
	const long total = (long)a.batch * a.blocks;
	for (long gb = blockIdx.x; gb < total; gb += gridDim.x) {
		const long b = gb / a.blocks;
		const int t = (int)(gb % a.blocks);
		const unsigned *const off = a.offsets + b * (a.blocks + 1);
		const unsigned o0 = off[t], o1 = off[t + 1];
		if (o1 == o0 || o1 > a.stream_stride)
			continue;
		const BlockRect r = block_rect(a, t);
		const int n = r.cw * r.ch, G = (n + 63) >> 6, nw = (int)(o1 - o0), p = nw / G - 1;
		const char *const src = a.index + b * a.bs + (long)r.y * a.pitch + (long)r.x * ES;
		u64 *const dst = a.words + (u64)b * a.stream_stride + o0;
		for (int wi = threadIdx.x; wi < nw; wi += 256) {
			const int k = wi / G, g = wi - k * G;
			u64 word = 0;
			for (int i = 64 * g; i < min(64 * g + 64, n); i++) {
				const int y = i / r.cw, x = i - y * r.cw;
				const int q = index_load<ES>(src + (long)y * a.pitch + (long)x * ES);
				const u64 bit = k == 0 ? (u64)(q < 0) : (u64)((magnitude(q) >> (p - k)) & 1u);
				word |= bit << (i & 63);
			}
			dst[wi] = word;
		}
	}
}

// What a block of a stream holds, from its two offsets: the magnitude planes p, 0 for a block of zeros and for a block
// that is written as zeros -- offsets not monotone, an end beyond the capacity, a length that is no multiple of G, more
// planes than the element type has bits.
template <int INDEX>
static __device__ __forceinline__ int stream_planes(unsigned o0, unsigned o1, u64 stream_stride, int G)
{
	constexpr unsigned PMAX = INDEX == kIndexI16 ? 16 : 32;
	if (o1 <= o0 || o1 > stream_stride)
		return 0;
	const unsigned len = o1 - o0, planes = len / (unsigned)G;
	if (planes * (unsigned)G != len || planes - 1 > PMAX)
		return 0;
	return (int)planes - 1;
}

// the element of magnitude bits m (|q| >> dk), the least significant dk planes left out
static __device__ __forceinline__ unsigned element_of(unsigned m, bool neg, int dk, int mode)
{
	const unsigned v = mode == kBitplaneKeep ? m << (dk & 31) : m; // (m != 0 only where dk < 32)
	return neg ? 0u - v : v;                                      // (0 stays 0 whatever the sign bit)
}

template <int INDEX>
__global__ __launch_bounds__(256) void k_bitplane_unpack(BitplaneArgs a)
{
	constexpr int ES = quant_index_es(INDEX);
	__shared__ u64 lds[BITPLANE_MAX_WORDS];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const long total = (long)a.batch * a.blocks;
	for (long gb = blockIdx.x; gb < total; gb += gridDim.x) {
		const long b = gb / a.blocks;
		const int t = (int)(gb % a.blocks);
		const unsigned *const off = a.offsets + b * (a.blocks + 1);
		const unsigned o0 = off[t], o1 = off[t + 1];
		const BlockRect r = block_rect(a, t);
		const int n = r.cw * r.ch, G = (n + 63) >> 6;
		const int p = stream_planes<INDEX>(o0, o1, a.stream_stride, G), dk = min(a.drop, p), keep = p - dk;
		const bool full = r.cw == (1 << a.cbx);
		if (keep > 0) {
			// the sign plane and the magnitude planes that are read: one contiguous run, inside [o0, o1)
			const u64 *const src = a.words + (u64)b * a.stream_stride + o0;
			const int nr = (keep + 1) * G, head = (int)(((uintptr_t)src >> 3) & 1), pairs = (nr - head) >> 1;
			for (int i = threadIdx.x; i < pairs; i += 256) {
				const u64x2 v = *(const u64x2 *)(src + head + 2 * i);
				lds[head + 2 * i] = v.x, lds[head + 2 * i + 1] = v.y;
			}
			if (threadIdx.x == 0 && head)
				lds[0] = src[0];
			if (threadIdx.x == 64 && ((nr - head) & 1))
				lds[nr - 1] = src[nr - 1];
		}
		__syncthreads();
		char *const dst = a.index + b * a.bs + (long)r.y * a.pitch + (long)r.x * ES;
		constexpr int RUN = 16 / ES;
		if (a.wide && ((long)r.x * ES) % 16 == 0 && r.cw % RUN == 0) {
			// Rows start on 16-byte boundaries and so do the block's rows: a lane takes a run of RUN consecutive samples of
			// a row -- RUN bits of one word of every plane -- and stores it by one 16-byte access; a wave RUN words a plane.
			for (int i = RUN * (int)threadIdx.x; i < n; i += RUN * 256) {
				const int g = i >> 6, sh = i & 63;
				unsigned m[RUN];
#pragma unroll
				for (int e = 0; e < RUN; e++)
					m[e] = 0;
				for (int k = 1; k <= keep; k++) {
					const unsigned bits = (unsigned)(lds[k * G + g] >> sh);
#pragma unroll
					for (int e = 0; e < RUN; e++)
						m[e] = (m[e] << 1) | ((bits >> e) & 1u);
				}
				const unsigned sign = keep > 0 ? (unsigned)(lds[g] >> sh) : 0u;
				unsigned out[RUN];
#pragma unroll
				for (int e = 0; e < RUN; e++)
					out[e] = element_of(m[e], (sign >> e) & 1u, dk, a.mode);
				const int y = full ? i >> a.cbx : i / r.cw, x = i - y * r.cw;
				run_store<ES>(dst + (long)y * a.pitch + (long)x * ES, out, a.nt != 0);
			}
			__syncthreads();
			continue;
		}
		for (int g = wave; g < G; g += 4) {
			const int i = 64 * g + lane;
			unsigned m = 0;
			for (int k = 1; k <= keep; k++)
				m = (m << 1) | (unsigned)((lds[k * G + g] >> lane) & 1u); // (one word for the wave: a broadcast)
			const bool neg = keep > 0 && ((lds[g] >> lane) & 1u);
			if (i < n) {
				const int y = full ? i >> a.cbx : i / r.cw, x = i - y * r.cw;
				index_store<ES>(dst + (long)y * a.pitch + (long)x * ES, element_of(m, neg, dk, a.mode), a.nt != 0);
			}
		}
		__syncthreads(); // (the next block's words go into the same LDS)
	}
}

template <int INDEX>
__global__ __launch_bounds__(256) void k_bitplane_unpack_plain(BitplaneArgs a)
{
	constexpr int ES = quant_index_es(INDEX);
	const long total = (long)a.batch * a.blocks;
	for (long gb = blockIdx.x; gb < total; gb += gridDim.x) {
		const long b = gb / a.blocks;
		const int t = (int)(gb % a.blocks);
		const unsigned *const off = a.offsets + b * (a.blocks + 1);
		const unsigned o0 = off[t], o1 = off[t + 1];
		const BlockRect r = block_rect(a, t);
		const int n = r.cw * r.ch, G = (n + 63) >> 6;
		const int p = stream_planes<INDEX>(o0, o1, a.stream_stride, G), dk = min(a.drop, p), keep = p - dk;
		const u64 *const src = a.words + (u64)b * a.stream_stride + o0; // (read only where keep > 0: inside [o0, o1))
		char *const dst = a.index + b * a.bs + (long)r.y * a.pitch + (long)r.x * ES;
		for (int g = threadIdx.x; g < G; g += 256) {
			const u64 sign = keep > 0 ? src[g] : 0;
			for (int i = 64 * g; i < min(64 * g + 64, n); i++) {
				unsigned m = 0;
				for (int k = 1; k <= keep; k++)
					m = (m << 1) | (unsigned)((src[k * G + g] >> (i & 63)) & 1u);
				const int y = i / r.cw, x = i - y * r.cw;
				index_store<ES>(dst + (long)y * a.pitch + (long)x * ES, element_of(m, (sign >> (i & 63)) & 1u, dk, a.mode), false);
			}
		}
	}
}

bool args_ok(int index, const BitplaneArgs &a)
{
	return (index == kIndexI16 || index == kIndexI32) && a.batch >= 1 && a.bands >= 1 && a.bands <= BAND_MAX_SLOTS && a.blocks >= 1 &&
	       a.first[a.bands] == a.blocks && a.cbx >= 2 && a.cby >= 2 && a.cbx <= 10 && a.cby <= 10 && a.cbx + a.cby <= 12 && a.index;
}

} // namespace

hipError_t launch_bitplane_sizes(int index, const BitplaneArgs &a, hipStream_t s)
{
	if (!args_ok(index, a) || !a.sizes)
		return hipErrorInvalidValue;
	// blocks past the cap are taken by the kernel's own loop (tests/test_hip_bitplanes.py)
	const long groups = ((long)a.batch * a.blocks + BITPLANE_WG_BLOCKS - 1) / BITPLANE_WG_BLOCKS;
	const unsigned grid = (unsigned)std::min<long>(groups, BITPLANE_GRID_BLOCKS);
	if (index == kIndexI16)
		k_bitplane_sizes<kIndexI16><<<grid, 256, 0, s>>>(a);
	else
		k_bitplane_sizes<kIndexI32><<<grid, 256, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_bitplane_scan(const BitplaneArgs &a, hipStream_t s)
{
	if (a.batch < 1 || a.blocks < 1 || !a.sizes || !a.offsets)
		return hipErrorInvalidValue;
	k_bitplane_scan<<<(unsigned)std::min(a.batch, BITPLANE_GRID_BATCH), 256, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_bitplane_pack(int index, bool wave, const BitplaneArgs &a, hipStream_t s)
{
	if (!args_ok(index, a) || !a.offsets || !a.words)
		return hipErrorInvalidValue;
	const unsigned grid = (unsigned)std::min<long>((long)a.batch * a.blocks, BITPLANE_GRID_BLOCKS);
	if (index == kIndexI16)
		wave ? k_bitplane_pack<kIndexI16><<<grid, 256, 0, s>>>(a) : k_bitplane_pack_plain<kIndexI16><<<grid, 256, 0, s>>>(a);
	else
		wave ? k_bitplane_pack<kIndexI32><<<grid, 256, 0, s>>>(a) : k_bitplane_pack_plain<kIndexI32><<<grid, 256, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_bitplane_unpack(int index, bool wave, const BitplaneArgs &a, hipStream_t s)
{
	if (!args_ok(index, a) || !a.offsets || !a.words || a.drop < 0 || a.drop > 32 || (a.mode != kBitplaneKeep && a.mode != kBitplaneShift))
		return hipErrorInvalidValue;
	const unsigned grid = (unsigned)std::min<long>((long)a.batch * a.blocks, BITPLANE_GRID_BLOCKS);
	if (index == kIndexI16)
		wave ? k_bitplane_unpack<kIndexI16><<<grid, 256, 0, s>>>(a) : k_bitplane_unpack_plain<kIndexI16><<<grid, 256, 0, s>>>(a);
	else
		wave ? k_bitplane_unpack<kIndexI32><<<grid, 256, 0, s>>>(a) : k_bitplane_unpack_plain<kIndexI32><<<grid, 256, 0, s>>>(a);
	return hipGetLastError();
}

} // namespace dwt
