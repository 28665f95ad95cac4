// dwt_wp1d.hip -- every level of a wavelet PACKET transform of a batch of lines in ONE launch (gfx950).
//
// The sibling of k_line_levels (dwt_line1d.hip).  A packet level splits EVERY node of the line, not only the L prefix:
// the node [s, s+n) of level j becomes L at [s, s+ceil(n/2)) and H right behind it (natural order, wp_node in
// dwt_kernels.h).  A line of up to N1D_MAX samples lies in LDS for all levels, so here it is read from HBM once, the
// levels ping-pong between two full-length LDS buffers, and the whole line is written once after the last level: 8 B of
// global traffic per float sample whatever the depth.
//
// Mapping: the threads-per-line rule and the load of k_line_levels.  At level j thread work is a SLOT (node q, pair k):
// every node gets P = ceil(longest node / 2) slots, slot p = q * P + k, so the (q, k) of a thread advance by constants
// from one iteration to the next -- two integer divisions per thread and level.  Uniform trees (N a multiple of
// 2^levels, the spectra case) take s = q * n by index arithmetic; any other N walks the j path bits of q (wp_node).
// Each pair is lifted from the 2K+1 register window of k_line_levels -- the same steps, end forms and scaling, reflected
// at the NODE's ends -- so the bits are those of the reference's one-level line function applied to each node.
// The level body is wp_level (dwt_wp_level.h), shared with the pruned-tree kernels of dwt_wp_basis.hip.
//
// LDS per line: 2 * r4(N) floats; 64 KiB at N1D_MAX, two workgroups per CU.
#include "dwt_kernels.h"
#include "dwt_lift.h"
#include "dwt_line_lds.h"
#include "dwt_device.h"
#include "dwt_wp_level.h"

namespace dwt {

template <class W, bool INV>
__global__ __launch_bounds__(256) void k_wp_lines(const char *__restrict__ src, char *__restrict__ dst, long line_stride,
	long elem_stride, int n_lines, int N, int levels, int tpl, int vec)
{
	using T = typename W::T;
	extern __shared__ float lds_f[];
	T *const lds = (T *)lds_f;
	const int sub = threadIdx.x / tpl, t = threadIdx.x % tpl;
	const int line = blockIdx.x * (blockDim.x / tpl) + sub;
	const bool active = line < n_lines;
	T *cur = lds + (long)sub * 2 * wp_r4(N);
	T *nxt = cur + wp_r4(N);
	const char *s = src + (long)line * line_stride;
	char *d = dst + (long)line * line_stride;
	const bool uniform = (N & ((1 << levels) - 1)) == 0;

	if (active)
		line_to_lds(cur, s, N, elem_stride, t, tpl, vec);

	for (int step = 0; step < levels; step++) {
		__syncthreads();
		const int lev = INV ? levels - 1 - step : step; // the level whose nodes are split (forward) / rebuilt (inverse)
		if (active)
			wp_level<W, INV, false>(cur, nxt, N, lev, t, tpl, uniform, nullptr);
		T *const x = cur;
		cur = nxt;
		nxt = x;
	}
	__syncthreads();
	if (!active)
		return;
	// the whole line, once
	wp_line_out(d, cur, N, elem_stride, t, tpl, vec);
}

template <class W>
static hipError_t wp_lines_t(bool inverse, const void *src, void *dst, long line_stride, long elem_stride, int n_lines, int N,
	int levels, hipStream_t s)
{
	// threads per line as k_line_levels: one wave for short lines (four lines per workgroup), the whole workgroup for long ones
	const int tpl = N <= 512 ? 64 : N <= 2048 ? 128 : 256;
	const int lpw = 256 / tpl;
	const size_t lds = (size_t)lpw * 2 * wp_r4(N) * sizeof(float);
	const int vec = elem_stride == 4 && line_stride % 16 == 0 && (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0;
	const dim3 grid((n_lines + lpw - 1) / lpw);
	if (inverse) {
		if (hipError_t e = allow_lds((const void *)k_wp_lines<W, true>, lds))
			return e;
		k_wp_lines<W, true><<<grid, 256, lds, s>>>((const char *)src, (char *)dst, line_stride, elem_stride, n_lines, N, levels, tpl, vec);
	} else {
		if (hipError_t e = allow_lds((const void *)k_wp_lines<W, false>, lds))
			return e;
		k_wp_lines<W, false><<<grid, 256, lds, s>>>((const char *)src, (char *)dst, line_stride, elem_stride, n_lines, N, levels, tpl, vec);
	}
	return hipGetLastError();
}

hipError_t launch_wp_lines(Wavelet w, bool inverse, const void *src, void *dst, long line_stride, long elem_stride, int n_lines,
	int N, int levels, hipStream_t s)
{
	if (n_lines <= 0)
		return hipSuccess;
	// (levels <= floor(log2 N): every node that is split has two samples or more)
	if (N < 2 || N > N1D_MAX || levels < 1 || (N >> levels) < 1 || elem_stride < 4 || elem_stride % 4)
		return hipErrorInvalidValue;
	switch (w) {
	case kCdf97S: return wp_lines_t<Cdf97S>(inverse, src, dst, line_stride, elem_stride, n_lines, N, levels, s);
	case kCdf53S: return wp_lines_t<Cdf53S>(inverse, src, dst, line_stride, elem_stride, n_lines, N, levels, s);
	case kInterp53S: return wp_lines_t<Interp53S>(inverse, src, dst, line_stride, elem_stride, n_lines, N, levels, s);
	default: return hipErrorInvalidValue;
	}
}

} // namespace dwt
