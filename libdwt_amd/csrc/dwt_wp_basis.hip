// dwt_wp_basis.hip -- pruned wavelet packet trees and the best-basis search of a batch of lines (gfx950).
//
// A tree is a bitmap of WP_TREE_WORDS words: bit h = 2^j + k set means that node k of level j is split; only the bits that
// can be reached from the root through set bits count (the EFFECTIVE tree), so no bitmap needs validation.
//
//   k_wp_tree   the transform of every line in its tree, ONE launch: the mapping, the load and the level body of
//               k_wp_lines (dwt_wp_level.h); at level j a slot of a node that is not split copies its two samples.
//   k_wp_best   the search, ONE launch.  Phase A runs the full tree and reduces, after the load and after every level, the
//               cost of every node of that level into a table of doubles in LDS.  Phase B selects bottom-up in LDS, one
//               thread per node and level.  Phase C reads the line from src again and runs the tree transform (in place
//               this is legal: dst has not been written yet).  12 B of global traffic per sample.
//   k_wp_cost_level, k_wp_select, k_wp_leaf_copy   the helpers of the cross-check route (dense frames, any
//               number of lines; dwt_backend_wp.hip).
//
// Cost sums are doubles in a FIXED order that depends on N and the level alone: a thread's strided partial sum, a xor
// butterfly inside the wave, the wave partials in wave order.  No float atomics; the same bits for every batch size and
// every position of the line in the batch.
//
// LDS per line of k_wp_best: 2 * r4(N) floats, 2^(levels+1) doubles, 4 doubles of wave partials, two bitmaps: 80.3 KiB at
// N1D_MAX and 10 levels, one workgroup per CU there.
#include "dwt_kernels.h"
#include "dwt_lift.h"
#include "dwt_line_lds.h"
#include "dwt_device.h"
#include "dwt_wp_level.h"
#include "dwt_wp_cost.h" // wp_term: one coefficient's term of a cost

#include <cfloat>
#include <climits>
#include <cmath>

namespace dwt {

// eff: the bits of raw below `levels` that can be reached from the root through set bits; threads 0 .. 31 of the line, one
// word each.  The caller puts a barrier on either side.
static __device__ __forceinline__ void wp_effective(const unsigned *raw, unsigned *eff, int levels, int t)
{
	if (t >= WP_TREE_WORDS)
		return;
	unsigned v = 0;
	for (int b = 0; b < 32; b++) {
		const int h = 32 * t + b;
		if (h < 1 || h >= (1 << levels))
			continue;
		bool on = true;
		for (int a = h; a >= 1 && on; a >>= 1)
			on = wp_tree_bit(raw, a);
		if (on)
			v |= 1u << b;
	}
	eff[t] = v;
}

// The cost of every node of level j of the line in buf -> tab[2^j + q], by the tpl threads of the line.  EVERY thread of
// the workgroup calls it (it holds barriers where a node is shared by several waves; the branches depend on j and tpl
// alone).  part: 4 doubles of the line.
static __device__ __forceinline__ void wp_level_costs(const float *buf, double *tab, double *part, int N, int j, int t, int tpl, bool uniform,
	int kind, float param)
{
	const int nn = 1 << j;
	if (nn >= tpl) { // a thread takes whole nodes
		for (int q = t; q < nn; q += tpl) {
			int s0 = q * (N >> j), n = N >> j;
			if (!uniform)
				wp_node(N, j, q, &s0, &n);
			double s = 0;
			for (int i = 0; i < n; i++)
				s += wp_term(kind, param, buf[s0 + i]);
			tab[nn + q] = s;
		}
		return;
	}
	const int g = tpl / nn; // threads of a node: a power of two, a part of a wave or whole waves
	const int q = t / g, r = t % g;
	int s0 = q * (N >> j), n = N >> j;
	if (!uniform)
		wp_node(N, j, q, &s0, &n);
	double s = 0;
	for (int i = r; i < n; i += g)
		s += wp_term(kind, param, buf[s0 + i]);
	const int gw = g < 64 ? g : 64;
	for (int m = 1; m < gw; m <<= 1)
		s += __shfl_xor(s, m);
	if (g <= 64) {
		if (r == 0)
			tab[nn + q] = s;
		return;
	}
	if ((t & 63) == 0)
		part[t >> 6] = s;
	__syncthreads();
	if (r == 0) {
		double v = part[t >> 6];
		for (int w = 1; w < (g >> 6); w++)
			v += part[(t >> 6) + w];
		tab[nn + q] = v;
	}
	__syncthreads();
}

template <class W, bool INV>
__global__ __launch_bounds__(256) void k_wp_tree(const char *__restrict__ src, char *__restrict__ dst, long line_stride, long elem_stride,
	int n_lines, int N, int levels, int tpl, int vec, const unsigned *__restrict__ tree, long tree_words)
{
	using T = typename W::T;
	extern __shared__ float lds_f[];
	T *const lds = (T *)lds_f;
	const int lpw = blockDim.x / tpl;
	const int sub = threadIdx.x / tpl, t = threadIdx.x % tpl;
	const int line = blockIdx.x * lpw + sub;
	const bool active = line < n_lines;
	T *cur = lds + (long)sub * 2 * wp_r4(N);
	T *nxt = cur + wp_r4(N);
	unsigned *const raw = (unsigned *)(lds_f + (long)lpw * 2 * wp_r4(N)) + sub * 2 * WP_TREE_WORDS, *const eff = raw + WP_TREE_WORDS;
	const bool uniform = (N & ((1 << levels) - 1)) == 0;

	if (t < WP_TREE_WORDS)
		raw[t] = active ? tree[(long)line * tree_words + t] : 0u;
	if (active)
		line_to_lds(cur, src + (long)line * line_stride, N, elem_stride, t, tpl, vec);
	__syncthreads();
	wp_effective(raw, eff, levels, t);
	for (int step = 0; step < levels; step++) {
		__syncthreads();
		const int lev = INV ? levels - 1 - step : step;
		if (active)
			wp_level<W, INV, true>(cur, nxt, N, lev, t, tpl, uniform, eff);
		T *const x = cur;
		cur = nxt;
		nxt = x;
	}
	__syncthreads();
	if (active)
		wp_line_out(dst + (long)line * line_stride, cur, N, elem_stride, t, tpl, vec);
}

template <class W>
__global__ __launch_bounds__(256) void k_wp_best(WpBestArgs a)
{
	using T = typename W::T;
	extern __shared__ float lds_f[];
	T *const lds = (T *)lds_f;
	const int N = a.N, levels = a.levels, tpl = a.tpl;
	const int lpw = blockDim.x / tpl;
	const int sub = threadIdx.x / tpl, t = threadIdx.x % tpl;
	const int line = blockIdx.x * lpw + sub;
	const bool active = line < a.n_lines;
	const int nt = 2 << levels; // entries of a line's table, heap order
	T *cur = lds + (long)sub * 2 * wp_r4(N);
	T *nxt = cur + wp_r4(N);
	double *const tabs = (double *)(lds_f + (long)lpw * 2 * wp_r4(N));
	double *const tab = tabs + (long)sub * nt;
	double *const part = tabs + (long)lpw * nt + sub * 4;
	unsigned *const raw = (unsigned *)(tabs + (long)lpw * (nt + 4)) + sub * 2 * WP_TREE_WORDS, *const eff = raw + WP_TREE_WORDS;
	const bool uniform = (N & ((1 << levels) - 1)) == 0;
	const char *const s = a.src + (long)line * a.line_stride;

	// phase A: the full tree, the costs of every node where its coefficients lie.  A line past the batch runs on what its
	// LDS holds: it meets every barrier and stores nothing.
	if (t < WP_TREE_WORDS)
		raw[t] = 0u;
	if (active)
		line_to_lds(cur, s, N, a.elem_stride, t, tpl, a.vec);
	__syncthreads();
	wp_level_costs(cur, tab, part, N, 0, t, tpl, uniform, a.kind, a.param);
	for (int lev = 0; lev < levels; lev++) {
		__syncthreads();
		wp_level<W, false, false>(cur, nxt, N, lev, t, tpl, uniform, nullptr);
		T *const x = cur;
		cur = nxt;
		nxt = x;
		__syncthreads();
		wp_level_costs(cur, tab, part, N, lev + 1, t, tpl, uniform, a.kind, a.param);
	}
	__syncthreads();
	if (active && a.node_cost)
		for (int h = 1 + t; h < nt; h += tpl)
			a.node_cost[(long)line * a.cost_doubles + h] = tab[h];

	// phase B: bottom-up, best[h] over cost[h] in place.  A tie and a NaN keep the parent.
	for (int j = levels - 1; j >= 0; j--) {
		__syncthreads();
		for (int q = t; q < (1 << j); q += tpl) {
			const int h = (1 << j) + q;
			const double c = tab[2 * h] + tab[2 * h + 1];
			if (c < tab[h]) {
				tab[h] = c;
				atomicOr(&raw[h >> 5], 1u << (h & 31));
			}
		}
	}
	__syncthreads();
	wp_effective(raw, eff, levels, t);
	if (active && t == 0) {
		if (a.total)
			a.total[line] = tab[1];
		if (a.node_cost)
			a.node_cost[(long)line * a.cost_doubles] = tab[1];
	}
	__syncthreads();
	if (active && a.tree && t < WP_TREE_WORDS)
		a.tree[(long)line * a.tree_words + t] = eff[t];
	if (!a.dst)
		return;

	// phase C: the line again, in the tree found
	if (active)
		line_to_lds(cur, s, N, a.elem_stride, t, tpl, a.vec);
	for (int lev = 0; lev < levels; lev++) {
		__syncthreads();
		if (active)
			wp_level<W, false, true>(cur, nxt, N, lev, t, tpl, uniform, eff);
		T *const x = cur;
		cur = nxt;
		nxt = x;
	}
	__syncthreads();
	if (active)
		wp_line_out(a.dst + (long)line * a.line_stride, cur, N, a.elem_stride, t, tpl, a.vec);
}

static int wp_tpl(int N) { return N <= 512 ? 64 : N <= 2048 ? 128 : 256; } // the rule of k_wp_lines

template <class W>
static hipError_t wp_tree_t(bool inverse, const void *src, void *dst, long line_stride, long elem_stride, int n_lines, int N, int levels,
	const unsigned *tree, long tree_words, hipStream_t s)
{
	const int tpl = wp_tpl(N), lpw = 256 / tpl;
	const size_t lds = (size_t)lpw * (2 * wp_r4(N) * sizeof(float) + 2 * WP_TREE_WORDS * sizeof(unsigned));
	const int vec = elem_stride == 4 && line_stride % 16 == 0 && (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0;
	const dim3 grid((n_lines + lpw - 1) / lpw);
	if (inverse) {
		if (hipError_t e = allow_lds((const void *)k_wp_tree<W, true>, lds))
			return e;
		k_wp_tree<W, true><<<grid, 256, lds, s>>>((const char *)src, (char *)dst, line_stride, elem_stride, n_lines, N, levels, tpl, vec, tree, tree_words);
	} else {
		if (hipError_t e = allow_lds((const void *)k_wp_tree<W, false>, lds))
			return e;
		k_wp_tree<W, false><<<grid, 256, lds, s>>>((const char *)src, (char *)dst, line_stride, elem_stride, n_lines, N, levels, tpl, vec, tree, tree_words);
	}
	return hipGetLastError();
}

static bool wp_tree_args_ok(int n_lines, int N, int levels, long elem_stride)
{
	return N >= 2 && N <= N1D_MAX && levels >= 1 && levels <= WP_TREE_MAX_LEVELS && (N >> levels) >= 1 && elem_stride >= 4 && elem_stride % 4 == 0;
}

hipError_t launch_wp_tree(Wavelet w, bool inverse, const void *src, void *dst, long line_stride, long elem_stride, int n_lines, int N,
	int levels, const unsigned *tree, long tree_words, hipStream_t s)
{
	if (n_lines <= 0)
		return hipSuccess;
	if (!wp_tree_args_ok(n_lines, N, levels, elem_stride) || !tree)
		return hipErrorInvalidValue;
	switch (w) {
	case kCdf97S: return wp_tree_t<Cdf97S>(inverse, src, dst, line_stride, elem_stride, n_lines, N, levels, tree, tree_words, s);
	case kCdf53S: return wp_tree_t<Cdf53S>(inverse, src, dst, line_stride, elem_stride, n_lines, N, levels, tree, tree_words, s);
	case kInterp53S: return wp_tree_t<Interp53S>(inverse, src, dst, line_stride, elem_stride, n_lines, N, levels, tree, tree_words, s);
	default: return hipErrorInvalidValue;
	}
}

template <class W>
static hipError_t wp_best_t(WpBestArgs a, hipStream_t s)
{
	a.tpl = wp_tpl(a.N);
	const int lpw = 256 / a.tpl;
	const size_t lds = (size_t)lpw * (2 * wp_r4(a.N) * sizeof(float) + ((2 << a.levels) + 4) * sizeof(double) + 2 * WP_TREE_WORDS * sizeof(unsigned));
	a.vec = a.elem_stride == 4 && a.line_stride % 16 == 0 && (uintptr_t)a.src % 16 == 0 && (uintptr_t)a.dst % 16 == 0;
	if (hipError_t e = allow_lds((const void *)k_wp_best<W>, lds))
		return e;
	k_wp_best<W><<<dim3((a.n_lines + lpw - 1) / lpw), 256, lds, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_wp_best(Wavelet w, const WpBestArgs &a, hipStream_t s)
{
	if (a.n_lines <= 0)
		return hipSuccess;
	if (!wp_tree_args_ok(a.n_lines, a.N, a.levels, a.elem_stride) || a.kind < kWpCostShannon || a.kind > kWpCostThreshold)
		return hipErrorInvalidValue;
	switch (w) {
	case kCdf97S: return wp_best_t<Cdf97S>(a, s);
	case kCdf53S: return wp_best_t<Cdf53S>(a, s);
	case kInterp53S: return wp_best_t<Interp53S>(a, s);
	default: return hipErrorInvalidValue;
	}
}

// ---- the helpers of the cross-check route: dense frames of n_lines rows, `pitch` bytes apart ------------------------------

// the cost of node q of level j of every line, one thread per (line, node), the node's terms in index order
__global__ __launch_bounds__(256) void k_wp_cost_level(const char *__restrict__ frame, long pitch, long n_lines, int N, int j, int kind,
	float param, double *__restrict__ tab, long tab_doubles)
{
	const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= (n_lines << j))
		return;
	const long line = i >> j;
	const int q = (int)(i & ((1 << j) - 1));
	int s0, n;
	wp_node(N, j, q, &s0, &n);
	const float *const p = (const float *)(frame + line * pitch) + s0;
	double s = 0;
	for (int k = 0; k < n; k++)
		s += wp_term(kind, param, p[k]);
	tab[line * tab_doubles + (1 << j) + q] = s;
}

// one thread per line: bottom-up over the line's table in place, the decisions into tree_ws (WP_TREE_WORDS words a line),
// made effective top-down; the total and the tree to the caller's outputs where given
__global__ __launch_bounds__(64) void k_wp_select(double *__restrict__ tab, long n_lines, int levels, unsigned *__restrict__ tree_ws,
	unsigned *__restrict__ tree, long tree_words, double *__restrict__ total, double *__restrict__ node_cost, long cost_doubles)
{
	const long line = (long)blockIdx.x * blockDim.x + threadIdx.x;
	if (line >= n_lines)
		return;
	double *const c = tab + line * (2l << levels);
	unsigned *const m = tree_ws + line * WP_TREE_WORDS;
	for (int k = 0; k < WP_TREE_WORDS; k++)
		m[k] = 0u;
	for (int h = (1 << levels) - 1; h >= 1; h--) {
		const double v = c[2 * h] + c[2 * h + 1];
		if (v < c[h]) {
			c[h] = v;
			m[h >> 5] |= 1u << (h & 31);
		}
	}
	for (int h = 2; h < (1 << levels); h++)
		if (!wp_tree_bit(m, h >> 1))
			m[h >> 5] &= ~(1u << (h & 31));
	if (total)
		total[line] = c[1];
	if (node_cost)
		node_cost[line * cost_doubles] = c[1];
	if (tree)
		for (int k = 0; k < WP_TREE_WORDS; k++)
			tree[line * tree_words + k] = m[k];
}

// One thread per sample.  The depth d of the sample's leaf: the walk from the root through set bits (a clear bit ends it,
// so unreachable bits are never read as splits).  mode 0 (forward, after level `lev` - 1 has been split): the sample is
// copied where d == lev; mode 1 (inverse, after the nodes of level `lev` have been rebuilt): where d <= lev, the spans of
// the nodes of that level that are not split.
__global__ __launch_bounds__(256) void k_wp_leaf_copy(const char *__restrict__ from, char *__restrict__ to, long pitch, long n_lines, int N,
	int levels, const unsigned *__restrict__ tree, long tree_words, int lev, int mode)
{
	const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n_lines * N)
		return;
	const long line = i / N;
	const int x = (int)(i % N);
	const unsigned *const m = tree + line * tree_words;
	int s = 0, n = N, h = 1, d = 0;
	while (d < levels && wp_tree_bit(m, h)) {
		const int nl = (n + 1) >> 1;
		if (x - s < nl) {
			n = nl;
			h = 2 * h;
		} else {
			s += nl;
			n -= nl;
			h = 2 * h + 1;
		}
		d++;
	}
	if (mode ? d <= lev : d == lev)
		*(float *)(to + line * pitch + 4l * x) = *(const float *)(from + line * pitch + 4l * x);
}

static unsigned blocks_for(long threads, int block) { return (unsigned)((threads + block - 1) / block); }

hipError_t launch_wp_cost_level(const void *frame, long pitch, long n_lines, int N, int j, int kind, float param, double *tab, long tab_doubles,
	hipStream_t s)
{
	if ((n_lines << j) > (long)INT_MAX * 128)
		return hipErrorInvalidValue;
	k_wp_cost_level<<<blocks_for(n_lines << j, 256), 256, 0, s>>>((const char *)frame, pitch, n_lines, N, j, kind, param, tab, tab_doubles);
	return hipGetLastError();
}

hipError_t launch_wp_select(double *tab, long n_lines, int levels, unsigned *tree_ws, unsigned *tree, long tree_words, double *total,
	double *node_cost, long cost_doubles, hipStream_t s)
{
	k_wp_select<<<blocks_for(n_lines, 64), 64, 0, s>>>(tab, n_lines, levels, tree_ws, tree, tree_words, total, node_cost, cost_doubles);
	return hipGetLastError();
}

hipError_t launch_wp_leaf_copy(const void *from, void *to, long pitch, long n_lines, int N, int levels, const unsigned *tree, long tree_words,
	int lev, int mode, hipStream_t s)
{
	if (n_lines * N > (long)INT_MAX * 128)
		return hipErrorInvalidValue;
	k_wp_leaf_copy<<<blocks_for(n_lines * N, 256), 256, 0, s>>>((const char *)from, (char *)to, pitch, n_lines, N, levels, tree, tree_words, lev, mode);
	return hipGetLastError();
}

} // namespace dwt
