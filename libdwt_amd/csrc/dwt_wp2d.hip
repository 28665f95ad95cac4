// dwt_wp2d.hip -- one level of a 2-D wavelet PACKET transform: every node of every image of a batch in ONE launch
// (gfx950).
//
// Level j of an image has 2^j x 2^j nodes, the product of the 1-D node rule (wp_node, dwt_kernels.h) along x and y.  A
// forward level gives every node what one level of the reference's 2-D driver gives an image of the node's size: every
// row lifted, then every column, LL | HL over LH | HH inside the node's own rectangle.  The inverse is that driver's
// inverse level: every row of the Mallat layout rebuilt, then every column (the float drivers undo rows first).
//
// k_wp2d_level: dense device images, out of place.  A workgroup of 256 lanes owns one tile of WP2D_TILE_W x WP2D_TILE_H
// samples (sample order) at an even origin inside one node:
//   1. it stages the tile plus K samples on every side in LDS, reflected at the NODE's borders (inverse: gathered from the
//      node's four quarters into sample order);
//   2. lifts every staged row horizontally, pair by pair from the 2K+1 register window of k_line_pass, into a second LDS
//      image;
//   3. lifts the tile's columns vertically from that image, the same window;
//   4. writes the four quarter tiles to the node's LL / HL / LH / HH places (inverse: the tile in sample order), adjacent
//      lanes to adjacent addresses.
// Windows, steps, end forms and scaling are those of k_line_pass on a line of the node's width / height, so the bits are
// those of the exact line passes (option "wp_fused" = 0).  Every sample of the frame belongs to one tile of one node, so a
// level writes the whole destination frame.  With the template flag TREE the same kernel runs a level of a pruned
// quadtree: a workgroup of a node that is not split copies its tile.
#include "dwt_kernels.h"
#include "dwt_lift.h"

#include <type_traits>

namespace dwt {

namespace {

constexpr int TW = WP2D_TILE_W, TH = WP2D_TILE_H;

// TREE: the workgroup derives, once, whether its node is split in the effective tree of its image -- the
// node's own bit and that of each of its at most 4 ancestors -- and lifts as above, or copies its tile from src to the same
// place in dst.  The nodes of a level under a leaf tile the leaf's rectangle, so the ping-pong of the levels keeps every leaf
// intact.  The bitmap decides lift-or-copy only, never an address.
template <class W, bool INV, bool TREE>
__global__ __launch_bounds__(256) void k_wp2d_level(std::conditional_t<TREE, Wp2dTreeArgs, Wp2dLevelArgs> a, int ntx, int nty)
{
	using T = typename W::T;
	constexpr int K = W::K;
	constexpr int F = INV ? 1 : (K & 1); // a window starts at sample 2k - K + F of its line
	constexpr int CW = TW + 2 * K, RH = TH + 2 * K;
	__shared__ T S1[RH][CW]; // the staged samples, sample order
	__shared__ T S2[RH][TW]; // ... after the row pass, sample order (pair k of a row at 2k, 2k + 1)
	const int tid = threadIdx.x;
	const int qx = blockIdx.x / ntx, tx = blockIdx.x % ntx, qy = blockIdx.y / nty, ty = blockIdx.y % nty;
	int sx, w, sy, h;
	wp_node(a.W, a.level, qx, &sx, &w);
	wp_node(a.H, a.level, qy, &sy, &h);
	const int x0 = tx * TW, y0 = ty * TH;
	if (x0 >= w || y0 >= h)
		return; // (a shorter node has fewer tiles; the whole workgroup leaves)
	// the tile's extent, rounded up to whole pairs: the last window of an odd extent reaches one sample further
	const int tw = min(TW, (w - x0 + 1) & ~1), th = min(TH, (h - y0 + 1) & ~1);
	const int wl = (w + 1) >> 1, hl = (h + 1) >> 1;
	const T *const src = (const T *)(a.src + (long)blockIdx.z * a.src_bs);
	T *const dst = (T *)(a.dst + (long)blockIdx.z * a.dst_bs);
	const long sp = a.src_pitch / 4, dp = a.dst_pitch / 4;
	if constexpr (TREE) {
		if (!wp_qtree_split(a.tree + (long)blockIdx.z * a.tree_words, a.level, qy, qx)) {
			for (int idx = tid; idx < TH * TW; idx += 256) {
				const int y = y0 + idx / TW, x = x0 + idx % TW;
				if (y < h && x < w)
					dst[(long)(sy + y) * dp + sx + x] = src[(long)(sy + y) * sp + sx + x];
			}
			return;
		}
	}

	// 1. stage
	const int rows = th + 2 * K, cols = tw + 2 * K;
	for (int idx = tid; idx < rows * CW; idx += 256) {
		const int i = idx / CW, c = idx % CW;
		if (c >= cols)
			continue;
		int y = y0 - K + i, x = x0 - K + c;
		if ((unsigned)y >= (unsigned)h)
			y = reflect(y, h);
		if ((unsigned)x >= (unsigned)w)
			x = reflect(x, w);
		if (INV) { // sample order -> the Mallat place inside the node
			y = (y & 1) ? hl + (y >> 1) : y >> 1;
			x = (x & 1) ? wl + (x >> 1) : x >> 1;
		}
		S1[i][c] = src[(long)(sy + y) * sp + sx + x];
	}
	__syncthreads();

	// 2. rows: pair kx of staged row i
	for (int idx = tid; idx < rows * (TW / 2); idx += 256) {
		const int i = idx / (TW / 2), kx = idx % (TW / 2);
		const int k = x0 / 2 + kx;
		if (2 * kx >= tw || 2 * k >= w)
			continue;
		const int g0 = 2 * k - K + F;
		T v[2 * K + 1];
#pragma unroll
		for (int j = 0; j <= 2 * K; j++) {
			const T raw = S1[i][2 * kx + F + j];
			v[j] = INV ? W::inv_scale((j + K + 1) & 1, raw) : raw; // (reflection keeps a sample's parity)
		}
		const unsigned ends = W::kEndForms ? end_mask<2 * K + 1>(g0, w) : 0u;
		if (INV) {
			lift_inv_regs<W, 2 * K + 1>(v, ends);
			S2[i][2 * kx] = v[K - 1];
			S2[i][2 * kx + 1] = v[K];
		} else {
			lift_fwd_regs<W, 2 * K + 1>(v, ends);
			S2[i][2 * kx] = W::fwd_scale(0, v[K - F]);
			S2[i][2 * kx + 1] = W::fwd_scale(1, v[K + 1 - F]);
		}
	}
	__syncthreads();

	// 3. columns, 4. store: pair ky of column c.  Forward: lanes 0 .. TW/2-1 of a row of work take the even columns (the L
	// half of the node), the others the odd ones, so that a wave's stores are contiguous in the quarter they go to.
	for (int idx = tid; idx < (TH / 2) * TW; idx += 256) {
		const int ky = idx / TW, m = idx % TW;
		const int c = INV ? m : (m < TW / 2 ? 2 * m : 2 * (m - TW / 2) + 1);
		const int k = y0 / 2 + ky, x = x0 + c;
		if (2 * ky >= th || 2 * k >= h || x >= w)
			continue;
		const int g0 = 2 * k - K + F;
		T v[2 * K + 1];
#pragma unroll
		for (int j = 0; j <= 2 * K; j++) {
			const T raw = S2[2 * ky + F + j][c];
			v[j] = INV ? W::inv_scale((j + K + 1) & 1, raw) : raw;
		}
		const unsigned ends = W::kEndForms ? end_mask<2 * K + 1>(g0, h) : 0u;
		if (INV) {
			lift_inv_regs<W, 2 * K + 1>(v, ends);
			T *const o = dst + (long)(sy + 2 * k) * dp + sx + x;
			o[0] = v[K - 1];
			if (2 * k + 1 < h)
				o[dp] = v[K];
		} else {
			lift_fwd_regs<W, 2 * K + 1>(v, ends);
			const int mx = (x & 1) ? wl + (x >> 1) : x >> 1;
			T *const o = dst + (long)(sy + k) * dp + sx + mx;
			o[0] = W::fwd_scale(0, v[K - F]);
			if (2 * k + 1 < h)
				o[(long)hl * dp] = W::fwd_scale(1, v[K + 1 - F]);
		}
	}
}

int tiles(int size, int level, int tile) { return wp_tiles(size, level, tile); } // per node along an axis: those of the longest node

template <class W>
hipError_t wp2d_level_t(bool inverse, const Wp2dLevelArgs &a, hipStream_t s)
{
	const int ntx = tiles(a.W, a.level, TW), nty = tiles(a.H, a.level, TH);
	const dim3 grid(ntx << a.level, nty << a.level, a.batch);
	if (inverse)
		k_wp2d_level<W, true, false><<<grid, 256, 0, s>>>(a, ntx, nty);
	else
		k_wp2d_level<W, false, false><<<grid, 256, 0, s>>>(a, ntx, nty);
	return hipGetLastError();
}

template <class W>
hipError_t wp2d_level_tree_t(bool inverse, const Wp2dTreeArgs &a, hipStream_t s)
{
	const int ntx = tiles(a.W, a.level, TW), nty = tiles(a.H, a.level, TH);
	const dim3 grid(ntx << a.level, nty << a.level, a.batch);
	if (inverse)
		k_wp2d_level<W, true, true><<<grid, 256, 0, s>>>(a, ntx, nty);
	else
		k_wp2d_level<W, false, true><<<grid, 256, 0, s>>>(a, ntx, nty);
	return hipGetLastError();
}

} // namespace

bool wp2d_level_fits(const Wp2dLevelArgs &a)
{
	if (a.W < 2 || a.H < 2 || a.batch < 1 || a.level < 0 || a.level > 7 || (a.W >> (a.level + 1)) < 1 || (a.H >> (a.level + 1)) < 1)
		return false;
	if ((uintptr_t)a.src % 4 || (uintptr_t)a.dst % 4 || a.src_pitch % 4 || a.dst_pitch % 4 || a.src_bs % 4 || a.dst_bs % 4)
		return false;
	return a.batch <= 65535 && ((long)tiles(a.H, a.level, TH) << a.level) <= 65535;
}

hipError_t launch_wp2d_level(Wavelet w, bool inverse, const Wp2dLevelArgs &a, hipStream_t s)
{
	if (!wp2d_level_fits(a) || a.src == a.dst)
		return hipErrorInvalidValue;
	switch (w) {
	case kCdf97S: return wp2d_level_t<Cdf97S>(inverse, a, s);
	case kCdf53S: return wp2d_level_t<Cdf53S>(inverse, a, s);
	case kInterp53S: return wp2d_level_t<Interp53S>(inverse, a, s);
	default: return hipErrorInvalidValue;
	}
}

hipError_t launch_wp2d_level_tree(Wavelet w, bool inverse, const Wp2dTreeArgs &a, hipStream_t s)
{
	if (!wp2d_level_fits(a) || a.src == a.dst || a.level >= WP_QTREE_MAX_LEVELS || !a.tree || (uintptr_t)a.tree % 4 || a.tree_words < 0)
		return hipErrorInvalidValue;
	switch (w) {
	case kCdf97S: return wp2d_level_tree_t<Cdf97S>(inverse, a, s);
	case kCdf53S: return wp2d_level_tree_t<Cdf53S>(inverse, a, s);
	case kInterp53S: return wp2d_level_tree_t<Interp53S>(inverse, a, s);
	default: return hipErrorInvalidValue;
	}
}

} // namespace dwt
