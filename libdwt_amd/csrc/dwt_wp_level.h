// dwt_wp_level.h -- one packet level of one line that lies in LDS: what k_wp_lines (dwt_wp1d.hip) and the tree kernels
// (dwt_wp_basis.hip) run between two barriers.  DESIGN.md s24 (the slot mapping), s28 (pruned trees).
#pragma once
#include "dwt_kernels.h"
#include "dwt_lift.h"

namespace dwt {

static __host__ __device__ __forceinline__ int wp_r4(int n) { return (n + 3) & ~3; }

// end_mask (dwt_lift.h) for the window of a pair of a node of n samples.  The deep levels of a tree are all short nodes,
// where end_mask reflects every entry with an integer division; but a window of m = 2K+1 samples around a pair of a node
// of n > m samples leaves the node by less than K + 2 on either side -- one bounce, which maps no other index onto sample
// 0 or n - 1 -- so there a sample is an end iff it IS one of the two (the form end_mask itself takes from 64 samples on).
template <int m>
static __device__ __forceinline__ unsigned node_end_mask(int g0, int n)
{
	return n > m ? end_mask_long<m>(g0, n) : end_mask<m>(g0, n);
}

// bit h of a tree bitmap (heap index h = 2^level + node; include/libdwt_hip.h)
static __host__ __device__ __forceinline__ bool wp_tree_bit(const unsigned *tree, int h) { return (tree[h >> 5] >> (h & 31)) & 1; }

// Level `lev` of the line in `cur` into `nxt`, by the `tpl` threads of the line (this one is t): every node of the level
// is split (forward) or rebuilt from its two children (INV).  Work is a SLOT (node q, pair k): every node gets
// P = ceil(longest node / 2) slots, slot p = q * P + k.  TREE: only the nodes whose bit is set in `split` (a bitmap of
// EFFECTIVE bits) are lifted; a slot of any other node copies its two samples.  The caller puts a barrier on either side.
template <class W, bool INV, bool TREE>
static __device__ __forceinline__ void wp_level(const typename W::T *cur, typename W::T *nxt, int N, int lev, int t, int tpl, bool uniform,
	const unsigned *split)
{
	using T = typename W::T;
	constexpr int K = W::K;
	const int nn = 1 << lev, a = N >> lev;
	const int P = (a + ((N & (nn - 1)) != 0) + 1) >> 1; // slots per node: pairs of the longest node
	int q = t / P, k = t % P;
	const int dq = tpl / P, dk = tpl % P;
	while (q < nn) {
		int s0 = q * a, n = a;
		if (!uniform)
			wp_node(N, lev, q, &s0, &n);
		const int nl = (n + 1) >> 1;
		if (k < nl) {
			T w[2 * K + 1];
			if (TREE && !wp_tree_bit(split, nn + q)) {
				nxt[s0 + 2 * k] = cur[s0 + 2 * k];
				if (2 * k + 1 < n)
					nxt[s0 + 2 * k + 1] = cur[s0 + 2 * k + 1];
			} else if (!INV) {
				constexpr int F = K & 1;
				const int g0 = 2 * k - K + F;
				const T *const in = cur + s0;
				if (g0 >= 0 && g0 + 2 * K < n) {
#pragma unroll
					for (int j = 0; j <= 2 * K; j++)
						w[j] = in[g0 + j];
				} else if (n > 2 * K + 1) {
#pragma unroll
					for (int j = 0; j <= 2 * K; j++)
						w[j] = in[reflect1(g0 + j, n)];
				} else {
#pragma unroll
					for (int j = 0; j <= 2 * K; j++)
						w[j] = in[reflect(g0 + j, n)];
				}
				lift_fwd_regs<W, 2 * K + 1>(w, W::kEndForms ? node_end_mask<2 * K + 1>(g0, n) : 0u);
				nxt[s0 + k] = W::fwd_scale(0, w[K - F]);
				if (2 * k + 1 < n)
					nxt[s0 + nl + k] = W::fwd_scale(1, w[K + 1 - F]);
			} else {
				const int g0 = 2 * k - K + 1;
				const T *const L = cur + s0, *const H = L + nl;
				const bool inner = g0 >= 0 && g0 + 2 * K < n;
#pragma unroll
				for (int j = 0; j <= 2 * K; j++) {
					const int i = inner ? g0 + j : n > 2 * K + 1 ? reflect1(g0 + j, n) : reflect(g0 + j, n);
					w[j] = W::inv_scale(i & 1, (i & 1) ? H[i >> 1] : L[i >> 1]);
				}
				lift_inv_regs<W, 2 * K + 1>(w, W::kEndForms ? node_end_mask<2 * K + 1>(g0, n) : 0u);
				nxt[s0 + 2 * k] = w[K - 1];
				if (2 * k + 1 < n)
					nxt[s0 + 2 * k + 1] = w[K];
			}
		}
		q += dq;
		k += dk;
		if (k >= P) {
			k -= P;
			q++;
		}
	}
}

// the line in LDS to its place in global memory, once
template <class T>
static __device__ __forceinline__ void wp_line_out(char *d, const T *cur, int N, long elem_stride, int t, int tpl, int vec)
{
	if (vec) {
		const int n4 = N >> 2;
		for (int i = t; i < n4; i += tpl)
			*(float4 *)(d + 16l * i) = *(const float4 *)(cur + 4 * i);
		for (int i = 4 * n4 + t; i < N; i += tpl)
			*(T *)(d + 4l * i) = cur[i];
	} else {
		for (int i = t; i < N; i += tpl)
			*(T *)(d + (long)i * elem_stride) = cur[i];
	}
}

} // namespace dwt
