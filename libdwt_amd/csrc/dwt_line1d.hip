// dwt_line1d.hip -- every level of a 1-D transform of a batch of lines in ONE launch (gfx950).
//
// The reference's 1-D drivers (dwt_cdf97_1f_s / _1i_s and the 5/3 siblings, src/libdwt.c:16025, :15766, :16097, :15835)
// run one exact line transform per level over the L prefix of the line.  A line of up to N1D_MAX samples fits in LDS,
// so here each line is read from HBM once, all levels run in LDS, and each coefficient is written once: 8 B of global
// traffic per float sample whatever the depth.
//
// Mapping: `T` threads per line (64 for short lines, so that several lines share a workgroup of 256 threads; 256 for
// long ones).  All lines of a launch have the same length and depth, so every thread meets the same barriers.
//
// Forward, level by level: the level's input (n samples) lies in LDS; thread k of the line takes output pair k with the
// 2K+1 taps around it -- the same window, the same steps, end forms and scaling as k_line_pass (dwt_sweep2d.hip), so the
// bits are those of the reference -- writes the H coefficient straight to its Mallat offset in global memory and the L
// coefficient to the other LDS buffer, the next level's input.  After the last level the final L part is stored.
//
// Inverse, the mirror: the whole line (L_J and every H band) is loaded at once -- the H loads do not wait for any
// lifting --, and each level reads its L part from the previous level's output and its H band from the loaded line,
// descales, lifts, and writes the next finer L part to LDS (the finest level: to global memory).
//
// LDS per line (floats, each part rounded up to 16 B): forward N + ceil(N/2), inverse N + ceil(N/2) + ceil(N/4).
// At N1D_MAX = 8192 the inverse takes 56 KiB: two workgroups per CU (160 KiB).
#include "dwt_kernels.h"
#include "dwt_lift.h"
#include "dwt_line_lds.h"

namespace dwt {

static __host__ __device__ __forceinline__ int r4(int n) { return (n + 3) & ~3; }
static __host__ __device__ __forceinline__ int div_pow2_up(int n, int j) { return (n + (1 << j) - 1) >> j; }

// floats of LDS one line takes
static __host__ __device__ __forceinline__ int line_lds_floats(bool inverse, int N)
{
	return r4(N) + r4(div_pow2_up(N, 1)) + (inverse ? r4(div_pow2_up(N, 2)) : 0);
}

template <class W, bool INV>
__global__ __launch_bounds__(256) void k_line_levels(const char *__restrict__ src, char *__restrict__ dst, long line_stride,
	long elem_stride, int n_lines, int N, int levels, int tpl, int vec)
{
	using T = typename W::T;
	constexpr int K = W::K;
	extern __shared__ float lds_f[];
	T *const lds = (T *)lds_f;
	const int sub = threadIdx.x / tpl, t = threadIdx.x % tpl;
	const int line = blockIdx.x * (blockDim.x / tpl) + sub;
	const bool active = line < n_lines;
	T *const A = lds + (long)sub * line_lds_floats(INV, N);
	T *const B = A + r4(N);
	T *const C = B + r4(div_pow2_up(N, 1));
	const char *s = src + (long)line * line_stride;
	char *d = dst + (long)line * line_stride;
	auto st = [&](int i, T v) { *(T *)(d + (long)i * elem_stride) = v; };

	if (active)
		line_to_lds(A, s, N, elem_stride, t, tpl, vec);

	if (!INV) {
		T *cur = A, *nxt = B;
		int n = N;
		for (int lev = 0; lev < levels; lev++) {
			__syncthreads();
			const int nl = (n + 1) >> 1;
			if (active) {
				if (n == 1) {
					if (t == 0)
						nxt[0] = W::kScaleSingle ? W::fwd_single(cur[0]) : cur[0];
				} else {
					for (int k = t; k < nl; k += tpl) {
						T w[2 * K + 1];
						// (F = 1: a policy of one step, whose window 2k .. 2k+2 starts at the even sample)
						constexpr int F = K & 1;
						const int g0 = 2 * k - K + F;
						if (g0 >= 0 && g0 + 2 * K < n) {
#pragma unroll
							for (int j = 0; j <= 2 * K; j++)
								w[j] = cur[g0 + j];
						} else {
#pragma unroll
							for (int j = 0; j <= 2 * K; j++)
								w[j] = cur[reflect(g0 + j, n)];
						}
						lift_fwd_regs<W, 2 * K + 1>(w, W::kEndForms ? end_mask<2 * K + 1>(g0, n) : 0u);
						nxt[k] = W::fwd_scale(0, w[K - F]);
						if (2 * k + 1 < n)
							st(nl + k, W::fwd_scale(1, w[K + 1 - F])); // H: final, to its Mallat offset
					}
				}
			}
			T *const x = cur;
			cur = nxt;
			nxt = x;
			n = nl;
		}
		__syncthreads();
		if (active)
			for (int i = t; i < n; i += tpl)
				st(i, cur[i]);
	} else {
		for (int lev = levels - 1; lev >= 0; lev--) {
			__syncthreads();
			const int n = div_pow2_up(N, lev), nl = div_pow2_up(N, lev + 1); // output length; L length = H offset
			const T *const L = (lev == levels - 1) ? A : ((lev + 1) & 1) ? B : C;
			const T *const H = A + nl;
			T *const out = (lev & 1) ? B : C; // (lev >= 1: B holds ceil(N/2), C ceil(N/4))
			if (!active)
				continue;
			if (n == 1) {
				if (t == 0) {
					const T v = W::kScaleSingle ? W::inv_single(L[0]) : L[0];
					if (lev == 0)
						st(0, v);
					else
						out[0] = v;
				}
				continue;
			}
			for (int k = t; k < nl; k += tpl) {
				T w[2 * K + 1];
				const int g0 = 2 * k - K + 1;
				const bool inner = g0 >= 0 && g0 + 2 * K < n;
#pragma unroll
				for (int j = 0; j <= 2 * K; j++) {
					const int i = inner ? g0 + j : reflect(g0 + j, n);
					w[j] = W::inv_scale(i & 1, (i & 1) ? H[i >> 1] : L[i >> 1]);
				}
				lift_inv_regs<W, 2 * K + 1>(w, W::kEndForms ? end_mask<2 * K + 1>(g0, n) : 0u);
				if (lev > 0) {
					out[2 * k] = w[K - 1];
					if (2 * k + 1 < n)
						out[2 * k + 1] = w[K];
				} else if (vec && 2 * k + 1 < n) {
					*(float2 *)(d + 8l * k) = make_float2(w[K - 1], w[K]);
				} else {
					st(2 * k, w[K - 1]);
					if (2 * k + 1 < n)
						st(2 * k + 1, w[K]);
				}
			}
		}
	}
}

template <class W>
static hipError_t line_levels_t(bool inverse, const void *src, void *dst, long line_stride, long elem_stride, int n_lines,
	int N, int levels, hipStream_t s)
{
	// threads per line: one wave for short lines (four lines per workgroup), the whole workgroup for long ones
	const int tpl = N <= 512 ? 64 : N <= 2048 ? 128 : 256;
	const int lpw = 256 / tpl;
	const size_t lds = (size_t)lpw * line_lds_floats(inverse, N) * sizeof(float);
	const int vec = elem_stride == 4 && line_stride % 16 == 0 && (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0;
	const dim3 grid((n_lines + lpw - 1) / lpw);
	if (inverse)
		k_line_levels<W, true><<<grid, 256, lds, s>>>((const char *)src, (char *)dst, line_stride, elem_stride, n_lines, N, levels, tpl, vec);
	else
		k_line_levels<W, false><<<grid, 256, lds, s>>>((const char *)src, (char *)dst, line_stride, elem_stride, n_lines, N, levels, tpl, vec);
	return hipGetLastError();
}

hipError_t launch_line_levels(Wavelet w, bool inverse, const void *src, void *dst, long line_stride, long elem_stride,
	int n_lines, int N, int levels, hipStream_t s)
{
	if (n_lines <= 0 || levels <= 0)
		return hipSuccess;
	if (N < 1 || N > N1D_MAX || levels > 31 || elem_stride < 4 || elem_stride % 4)
		return hipErrorInvalidValue;
	switch (w) {
	case kCdf97S: return line_levels_t<Cdf97S>(inverse, src, dst, line_stride, elem_stride, n_lines, N, levels, s);
	case kCdf53S: return line_levels_t<Cdf53S>(inverse, src, dst, line_stride, elem_stride, n_lines, N, levels, s);
	case kInterp53S: return line_levels_t<Interp53S>(inverse, src, dst, line_stride, elem_stride, n_lines, N, levels, s);
	default: return hipErrorInvalidValue;
	}
}

} // namespace dwt
