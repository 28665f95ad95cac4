// dwt_wp_basis2d.hip -- the best-basis search over packet QUADTREES of image batches: costs, the selection, and the copy
// helper of the cross-check route (gfx950).  The transform in a tree is k_wp2d_level<.., TREE> (dwt_wp2d.hip).
//
// A tree is a bitmap of WP_QTREE_WORDS words: bit q = (4^j - 1)/3 + ky*2^j + kx set means that node (ky, kx) of level j is
// split into LL, HL, LH, HH; only the bits that can be reached from the root through set bits count (the EFFECTIVE tree).
//
//   k_wp_qcost_tiles   the grid of k_wp2d_level (tiles x nodes, batch along z): a workgroup reduces the terms of its tile
//                      of its node to ONE double -- a strided partial per lane, a xor butterfly on doubles inside the wave,
//                      the four wave partials through LDS in wave order -- and writes it to the tile's own slot.
//   k_wp_qselect       one workgroup per image, one thread per node: the node's tile partials added in tile-index order
//                      into the cost table, then the selection bottom-up on a copy of the table in LDS, the decisions made
//                      effective top-down; tree, total and table written for all images in one launch.
//   k_wp_qcost_level, k_wp_qleaf_copy   the cross-check route's: one thread per (image, node) / per sample, 64-bit
//                      indices on 1-D grids.
//
// Cost sums are doubles in a FIXED order that depends on the image's size, the level and the node alone.  No float or
// double atomics (the bitmaps take integer atomics in LDS); the same bits for every batch size and every position of the
// image in the batch.
#include "dwt_kernels.h"
#include "dwt_wp_cost.h"

#include <climits>

namespace dwt {

namespace {

constexpr int TW = WP2D_TILE_W, TH = WP2D_TILE_H;
constexpr int QNODES_MAX = (4 * (1 << (2 * WP_QTREE_MAX_LEVELS)) - 1) / 3; // 1365: the nodes of levels 0 .. 5

__global__ __launch_bounds__(256) void k_wp_qcost_tiles(WpQCostArgs a, int ntx, int nty)
{
	__shared__ double wave[4];
	const int tid = threadIdx.x;
	const int qx = blockIdx.x / ntx, tx = blockIdx.x % ntx, qy = blockIdx.y / nty, ty = blockIdx.y % nty;
	int sx, w, sy, h;
	wp_node(a.W, a.level, qx, &sx, &w);
	wp_node(a.H, a.level, qy, &sy, &h);
	const int x0 = tx * TW, y0 = ty * TH;
	if (x0 >= w || y0 >= h)
		return; // (a shorter node has fewer tiles; the selection reads the slots of the node's own tiles only)
	const char *const img = a.frame + (long)blockIdx.z * a.bs;
	double s = 0;
	for (int idx = tid; idx < TH * TW; idx += 256) {
		const int y = y0 + idx / TW, x = x0 + idx % TW;
		if (y < h && x < w)
			s += wp_term(a.kind, a.param, *(const float *)(img + (long)(sy + y) * a.pitch + 4l * (sx + x)));
	}
	for (int m = 1; m < 64; m <<= 1)
		s += __shfl_xor(s, m);
	if ((tid & 63) == 0)
		wave[tid >> 6] = s;
	__syncthreads();
	if (tid == 0) {
		const long node = ((long)qy << a.level) + qx;
		a.part[(long)blockIdx.z * a.part_stride + (node * nty + ty) * ntx + tx] = ((wave[0] + wave[1]) + wave[2]) + wave[3];
	}
}

// level, ky, kx of the quadtree index q
__device__ __forceinline__ void q_decode(int q, int *j, int *ky, int *kx)
{
	int l = 0;
	while (q >= wp_qbase(l + 1))
		l++;
	const int r = q - wp_qbase(l);
	*j = l, *ky = r >> l, *kx = r & ((1 << l) - 1);
}

__global__ __launch_bounds__(256) void k_wp_qselect(WpQSelectArgs a)
{
	__shared__ double best[QNODES_MAX];
	__shared__ unsigned bits[WP_QTREE_WORDS];
	const int tid = threadIdx.x, L = a.levels;
	const long b = blockIdx.x;
	const int nq = wp_qbase(L + 1);
	double *const tab = a.tab + b * nq;
	if (tid < WP_QTREE_WORDS)
		bits[tid] = 0u;
	for (int q = tid; q < nq; q += 256) {
		double c;
		if (a.part) {
			int j, ky, kx, sx, w, sy, h;
			q_decode(q, &j, &ky, &kx);
			wp_node(a.W, j, kx, &sx, &w);
			wp_node(a.H, j, ky, &sy, &h);
			const int ntx = wp_tiles(a.W, j, TW), nty = wp_tiles(a.H, j, TH);
			const double *const p = a.part + b * a.part_stride + a.part_off[j] + (((long)ky << j) + kx) * nty * ntx;
			c = 0;
			for (int ty = 0; ty < (h + TH - 1) / TH; ty++)
				for (int tx = 0; tx < (w + TW - 1) / TW; tx++)
					c += p[(long)ty * ntx + tx];
			tab[q] = c;
		} else
			c = tab[q];
		best[q] = c;
		if (a.node_cost)
			a.node_cost[b * a.cost_doubles + q] = c;
	}
	// bottom-up: a tie and a NaN keep the parent
	for (int j = L - 1; j >= 0; j--) {
		__syncthreads();
		for (int r = tid; r < (1 << (2 * j)); r += 256) {
			const int ky = r >> j, kx = r & ((1 << j) - 1), q = wp_qbase(j) + r;
			const int ll = wp_qbase(j + 1) + ((2 * ky) << (j + 1)) + 2 * kx, lh = ll + (2 << j);
			const double c = ((best[ll] + best[ll + 1]) + best[lh]) + best[lh + 1];
			if (c < best[q]) {
				best[q] = c;
				atomicOr(&bits[q >> 5], 1u << (q & 31));
			}
		}
	}
	// top-down: a set bit under a clear one is dropped
	for (int j = 1; j < L; j++) {
		__syncthreads();
		for (int r = tid; r < (1 << (2 * j)); r += 256) {
			const int ky = r >> j, kx = r & ((1 << j) - 1), q = wp_qbase(j) + r;
			const int up = wp_qbase(j - 1) + ((ky >> 1) << (j - 1)) + (kx >> 1);
			if (!((bits[up >> 5] >> (up & 31)) & 1u))
				atomicAnd(&bits[q >> 5], ~(1u << (q & 31)));
		}
	}
	__syncthreads();
	if (tid < WP_QTREE_WORDS) {
		a.tree_ws[b * WP_QTREE_WORDS + tid] = bits[tid];
		if (a.tree)
			a.tree[b * a.tree_words + tid] = bits[tid];
	}
	if (tid == 0 && a.total)
		a.total[b] = best[0];
}

__global__ __launch_bounds__(256) void k_wp_qcost_level(const char *__restrict__ frame, long pitch, long bs, int W, int H, long batch, int level,
	int kind, float param, double *__restrict__ tab, long tab_doubles)
{
	const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= (batch << (2 * level)))
		return;
	const long b = i >> (2 * level);
	const int r = (int)(i & ((1 << (2 * level)) - 1)), ky = r >> level, kx = r & ((1 << level) - 1);
	int sx, w, sy, h;
	wp_node(W, level, kx, &sx, &w);
	wp_node(H, level, ky, &sy, &h);
	double s = 0;
	for (int y = 0; y < h; y++) {
		const float *const p = (const float *)(frame + b * bs + (long)(sy + y) * pitch) + sx;
		for (int x = 0; x < w; x++)
			s += wp_term(kind, param, p[x]);
	}
	tab[b * tab_doubles + wp_qbase(level) + r] = s;
}

// The depth d of the sample's leaf: the walk from the root through set bits (a clear bit ends it, so unreachable bits are
// never read as splits).  mode 0 (forward, after level `lev` - 1 has been split): the sample is copied where d == lev; mode 1
// (inverse, after the nodes of level `lev` have been rebuilt): where d <= lev, the rectangles of the nodes of that level
// that are not split.
__global__ __launch_bounds__(256) void k_wp_qleaf_copy(const char *__restrict__ from, char *__restrict__ to, long pitch, long bs, int W, int H,
	long batch, int levels, const unsigned *__restrict__ tree, long tree_words, int lev, int mode)
{
	const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= batch * H * W)
		return;
	const long b = i / ((long)H * W);
	const int y = (int)(i / W % H), x = (int)(i % W);
	const unsigned *const m = tree + b * tree_words;
	int sx = 0, w = W, sy = 0, h = H, ky = 0, kx = 0, d = 0;
	while (d < levels) {
		const int q = wp_qbase(d) + (ky << d) + kx;
		if (!((m[q >> 5] >> (q & 31)) & 1u))
			break;
		const int wl = (w + 1) >> 1, hl = (h + 1) >> 1;
		kx *= 2, ky *= 2;
		if (x - sx < wl)
			w = wl;
		else
			sx += wl, w -= wl, kx++;
		if (y - sy < hl)
			h = hl;
		else
			sy += hl, h -= hl, ky++;
		d++;
	}
	if (mode ? d <= lev : d == lev) {
		const long off = b * bs + (long)y * pitch + 4l * x;
		*(float *)(to + off) = *(const float *)(from + off);
	}
}

unsigned blocks_for(long threads, int block) { return (unsigned)((threads + block - 1) / block); }

bool shape_ok(int W, int H, long batch, int level)
{
	return W >= 2 && H >= 2 && batch >= 1 && level >= 0 && level <= WP_QTREE_MAX_LEVELS && (W >> level) >= 1 && (H >> level) >= 1;
}

} // namespace

hipError_t launch_wp_qcost_tiles(const WpQCostArgs &a, hipStream_t s)
{
	if (!shape_ok(a.W, a.H, a.batch, a.level) || a.kind < kWpCostShannon || a.kind > kWpCostThreshold || !a.frame || !a.part)
		return hipErrorInvalidValue;
	if ((uintptr_t)a.frame % 4 || a.pitch % 4 || a.bs % 4 || (uintptr_t)a.part % 8)
		return hipErrorInvalidValue;
	const int ntx = wp_tiles(a.W, a.level, TW), nty = wp_tiles(a.H, a.level, TH);
	if (a.batch > 65535 || ((long)nty << a.level) > 65535)
		return hipErrorInvalidValue;
	k_wp_qcost_tiles<<<dim3(ntx << a.level, nty << a.level, a.batch), 256, 0, s>>>(a, ntx, nty);
	return hipGetLastError();
}

hipError_t launch_wp_qcost_level(const void *frame, long pitch, long bs, int W, int H, long batch, int level, int kind, float param, double *tab,
	long tab_doubles, hipStream_t s)
{
	if (!shape_ok(W, H, batch, level) || (batch << (2 * level)) > (long)INT_MAX * 128)
		return hipErrorInvalidValue;
	k_wp_qcost_level<<<blocks_for(batch << (2 * level), 256), 256, 0, s>>>((const char *)frame, pitch, bs, W, H, batch, level, kind, param, tab,
		tab_doubles);
	return hipGetLastError();
}

hipError_t launch_wp_qselect(const WpQSelectArgs &a, hipStream_t s)
{
	if (a.levels < 1 || a.levels > WP_QTREE_MAX_LEVELS || !shape_ok(a.W, a.H, a.batch, a.levels) || !a.tab || !a.tree_ws)
		return hipErrorInvalidValue;
	k_wp_qselect<<<dim3(a.batch), 256, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_wp_qleaf_copy(const void *from, void *to, long pitch, long bs, int W, int H, long batch, int levels, const unsigned *tree,
	long tree_words, int lev, int mode, hipStream_t s)
{
	if (!shape_ok(W, H, batch, 0) || levels < 1 || levels > WP_QTREE_MAX_LEVELS || batch * H * W > (long)INT_MAX * 128)
		return hipErrorInvalidValue;
	k_wp_qleaf_copy<<<blocks_for(batch * H * W, 256), 256, 0, s>>>((const char *)from, (char *)to, pitch, bs, W, H, batch, levels, tree, tree_words, lev,
		mode);
	return hipGetLastError();
}

} // namespace dwt
