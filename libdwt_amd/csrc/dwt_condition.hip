// dwt_condition.hip -- the kernels that condition a batch of rows before a transform, as the reference's spectra programs
// do (dwt_util_shift21_med_s, dwt_util_center21_s, dwt_util_scale21_s and their primitives, src/libdwt.c:25426-26055):
// subtract each row's median, move each row until its centre (dwt_cond_center.h) lies at n/2, map each row's range to
// [lo, hi].  DESIGN.md s16.
//
// k_cond_lines: dense rows of up to N1D_MAX samples, all three operations in ONE launch.  A workgroup takes `rows` rows
// into LDS (as many as the LDS holds); its waves select the medians and form the terms |x - med|^10 in parallel, one row
// per wave at a time; then lane r of wave 0 runs the serial float chains of row r -- a centre evaluation is up to 3n
// dependent additions (the sum, then two scans that stop at their crossing), so the rows of a workgroup run theirs side
// by side, one per lane.  A move is never carried out during the iterations: a row is (offset, first kept, last kept + 1) over its terms, the zero-filled samples being exact
// +0 terms.  The samples themselves are read once more at the end, shifted into LDS, scaled there and stored once.
//
// The per-operation kernels (median, min / max, centre, displace, shift, scale of rows in global memory) serve longer
// rows and large batches (every row of the batch is in flight there, one per lane, where the fused kernel keeps only what
// the LDS of a CU holds) and are what option "cond_fused" = 0 runs: the cross-check of the fused kernel, bit for bit.
#include "dwt_device.h"
#include "dwt_kernels.h"
#include "dwt_line_lds.h"

namespace dwt {

namespace {

#include "dwt_feat_acc.h"
#include "dwt_cond_center.h"

// the two separately rounded operations of dwt_util_scale21_s on one sample; the quotient of two floats taken in double
// and rounded to float is the correctly rounded float quotient (53 >= 2*24 + 2)
static __device__ __forceinline__ float scale_add(float lo, float mn) { return lo - mn; }
static __device__ __forceinline__ float scale_mul(float lo, float hi, float mn, float mx)
{
	return (float)((double)(hi - lo) / (double)(mx - mn));
}

constexpr int kCondMaxRows = 64; // rows of one workgroup: one lane of wave 0 each

__global__ __launch_bounds__(256) void k_cond_lines(CondLineArgs a)
{
	extern __shared__ __attribute__((aligned(16))) float cl[];
	__shared__ unsigned hist[4][256];
	__shared__ float s_nm[kCondMaxRows]; // -median
	__shared__ int s_off[kCondMaxRows], s_lo[kCondMaxRows], s_hi[kCondMaxRows], s_moves[kCondMaxRows], s_c[kCondMaxRows], s_skip[kCondMaxRows];
	const int t = threadIdx.x, w = t >> 6, l = t & 63, N = a.N;
	const int rs = ((N + 3) & ~3) + 4; // floats between the rows in LDS: 16-byte aligned, neighbours four banks apart
	const long row0 = (long)blockIdx.x * a.rows;
	const int nr = (int)min((long)a.rows, a.n_lines - row0);
	const bool med = (a.ops & kCondMedShift) != 0, center = (a.ops & kCondCenter) != 0 && a.max_iters > 0;
	for (int r = w; r < nr; r += 4)
		line_to_lds(cl + r * rs, a.ptr + (row0 + r) * a.line_stride, N, 4, l, 64, a.vec != 0);
	if (t < kCondMaxRows) {
		s_nm[t] = 0.f;
		s_off[t] = 0;
		s_lo[t] = 0;
		s_hi[t] = N;
		s_moves[t] = 0;
		s_c[t] = -1;
		s_skip[t] = 0;
	}
	__syncthreads();
	// ---- the median: the radix select of reduce_record (dwt_feat_acc.h), a wave per row; every wave meets every barrier
	if (med) {
		for (int r0 = 0; r0 < nr; r0 += 4) {
			const int r = r0 + w;
			const bool act = r < nr;
			float *row = cl + (act ? r : 0) * rs;
			unsigned prefix = 0, rank = (unsigned)N / 2;
			for (int pass = 0; pass < 4; pass++) {
				const int shift = 24 - 8 * pass;
				for (int i = l; i < 256; i += 64)
					hist[w][i] = 0;
				__syncthreads();
				if (act)
					for (int i = l; i < N; i += 64) {
						const unsigned q = okey(row[i]);
						if (pass == 0 || (q >> (shift + 8)) == prefix)
							atomicAdd(&hist[w][(q >> shift) & 255], 1u);
					}
				__syncthreads();
				unsigned kk = rank;
				const unsigned bin = pick_bin(hist[w], &kk);
				prefix = (prefix << 8) | bin;
				rank = kk;
				__syncthreads();
			}
			if (act) {
				const float nm = -okey_inv(prefix);
				if (!center) // (else the samples are read again below)
					for (int i = l; i < N; i += 64)
						row[i] += nm;
				if (l == 0)
					s_nm[r] = nm;
			}
		}
		__syncthreads();
	}
	if (center) {
		// ---- the terms, in parallel
		for (int r = w; r < nr; r += 4) {
			float *row = cl + r * rs;
			const float nm = s_nm[r];
			for (int i = l; i < N; i += 64)
				row[i] = cond_term(med ? row[i] + nm : row[i]);
		}
		__syncthreads();
		// ---- the chains: row t on lane t.  The row is cur[x] = lo <= x < hi ? sample[x + off] : 0
		if (t < nr) {
			const float *tr = cl + t * rs;
			int off = 0, lo = 0, hi = N, moves = 0, c = -1, wn = 0, wi = 0;
			for (int it = 0; it < a.max_iters; it++) {
				int warn;
				c = cond_center(N, lo, hi, [&](int x) { return tr[x + off]; }, &warn);
				wn += warn == kCondWarnNorm;
				wi += warn == kCondWarnIndex;
				const int d = c - N / 2; // displace1_zero(row, -(n/2 - c)): new[x] = cur[x + d]
				if (!d)
					break;
				off += d;
				lo = max(lo - d, 0);
				hi = max(min(hi - d, N), lo);
				moves++;
			}
			s_off[t] = off;
			s_lo[t] = lo;
			s_hi[t] = hi;
			s_moves[t] = moves;
			s_c[t] = c;
			if (wn)
				atomicAdd(a.warn, wn);
			if (wi)
				atomicAdd(a.warn + 1, wi);
		}
		__syncthreads();
		// ---- the moved rows, from the samples themselves (lo + off >= 0 and hi + off <= N by construction)
		for (int r = w; r < nr; r += 4) {
			float *row = cl + r * rs;
			const float *gr = (const float *)(a.ptr + (row0 + r) * a.line_stride);
			const int off = s_off[r], lo = s_lo[r], hi = s_hi[r];
			const float nm = s_nm[r];
			for (int i = l; i < N; i += 64) {
				float v = 0.0f;
				if (i >= lo && i < hi) {
					v = gr[i + off];
					if (med)
						v += nm;
				}
				row[i] = v;
			}
		}
		__syncthreads();
	}
	if (a.ops & kCondScale) {
		for (int r = w; r < nr; r += 4) {
			float *row = cl + r * rs;
			float mn = row[0], mx = row[0];
			for (int i = l; i < N; i += 64) {
				mn = fminf(mn, row[i]);
				mx = fmaxf(mx, row[i]);
			}
#pragma unroll
			for (int o = 32; o > 0; o >>= 1) {
				mn = fminf(mn, __shfl_xor(mn, o));
				mx = fmaxf(mx, __shfl_xor(mx, o));
			}
			if (mx == mn) {
				if (l == 0)
					s_skip[r] = 1;
			} else {
				const float add = scale_add(a.lo, mn), mul = scale_mul(a.lo, a.hi, mn, mx);
				for (int i = l; i < N; i += 64)
					row[i] = (row[i] + add) * mul;
			}
		}
	}
	__syncthreads();
	for (int r = w; r < nr; r += 4) {
		const float *row = cl + r * rs;
		char *g = a.ptr + (row0 + r) * a.line_stride;
		if (a.vec) {
			const int n4 = N >> 2;
			for (int i = l; i < n4; i += 64)
				*(float4 *)(g + 16l * i) = *(const float4 *)(row + 4 * i);
			for (int i = 4 * n4 + l; i < N; i += 64)
				*(float *)(g + 4l * i) = row[i];
		} else {
			for (int i = l; i < N; i += 64)
				*(float *)(g + 4l * i) = row[i];
		}
	}
	if (a.info && t < nr) {
		int *o = a.info + 4 * (row0 + t);
		o[0] = s_off[t];
		o[1] = s_moves[t];
		o[2] = s_c[t];
		o[3] = s_skip[t];
	}
}

// ---- the per-operation kernels: rows in global memory, sample i of row y at p + y*ls + 4*i ------------------------------
__global__ __launch_bounds__(256) void k_rows_median(const char *p, long ls, int N, float *med)
{
	__shared__ unsigned hist[256];
	__shared__ unsigned sel[2];
	const int t = threadIdx.x;
	const float *row = (const float *)(p + (long)blockIdx.x * ls);
	unsigned prefix = 0, rank = (unsigned)N / 2;
	for (int pass = 0; pass < 4; pass++) {
		const int shift = 24 - 8 * pass;
		hist[t] = 0;
		__syncthreads();
		for (int i = t; i < N; i += 256) {
			const unsigned q = okey(row[i]);
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
	if (t == 0)
		med[blockIdx.x] = okey_inv(prefix);
}

__global__ __launch_bounds__(256) void k_rows_minmax(const char *p, long ls, int N, float *mn_out, float *mx_out)
{
	__shared__ float sh[8];
	const int t = threadIdx.x;
	const float *row = (const float *)(p + (long)blockIdx.x * ls);
	float mn = row[0], mx = row[0];
	for (int i = t; i < N; i += 256) {
		mn = fminf(mn, row[i]);
		mx = fmaxf(mx, row[i]);
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) {
		mn = fminf(mn, __shfl_xor(mn, o));
		mx = fmaxf(mx, __shfl_xor(mx, o));
	}
	if ((t & 63) == 0) {
		sh[t >> 6] = mn;
		sh[4 + (t >> 6)] = mx;
	}
	__syncthreads();
	if (t == 0) {
		mn_out[blockIdx.x] = fminf(fminf(sh[0], sh[1]), fminf(sh[2], sh[3]));
		mx_out[blockIdx.x] = fmaxf(fmaxf(sh[4], sh[5]), fmaxf(sh[6], sh[7]));
	}
}

// one thread per row.  center: the centre; displ (optional): c - n/2, the move center1 would make next; info (optional):
// the row's record updated as by one iteration; moved (optional): set when any row moves; warn: two counters.  skip_done:
// a row whose displ is 0 has converged in an earlier iteration and is not looked at again, as center1 stops there
__global__ __launch_bounds__(64) void k_rows_center(const char *p, long ls, int n_lines, int N, int *center, int *displ, int *info, int *moved,
	int *warn, int skip_done)
{
	const int y = blockIdx.x * 64 + threadIdx.x;
	if (y >= n_lines || (skip_done && displ[y] == 0))
		return;
	const float *row = (const float *)(p + (long)y * ls);
	int w;
	const int c = cond_center(N, 0, N, [&](int x) { return cond_term(row[x]); }, &w);
	if (w)
		atomicAdd(warn + (w == kCondWarnIndex), 1);
	const int d = c - N / 2;
	center[y] = c;
	if (displ)
		displ[y] = d;
	if (info) {
		info[4 * y + 2] = c;
		if (d) {
			info[4 * y] += d;
			info[4 * y + 1] += 1;
		}
	}
	if (moved && d)
		*moved = 1;
}

// dst[x] = src[x + d] inside the row; outside: zero, or the nearest sample (dwt_util_displace1_zero_s / displace1_s)
__global__ __launch_bounds__(256) void k_rows_displace(const char *src, long sls, char *dst, long dls, int n_lines, int N, const int *displ, int displ_all, int zero_fill)
{
	const int x = blockIdx.x * 256 + threadIdx.x;
	if (x >= N)
		return;
	for (int y = blockIdx.y; y < n_lines; y += gridDim.y) {
		const float *s = (const float *)(src + (long)y * sls);
		const long q = (long)x + (displ ? displ[y] : displ_all);
		const long qc = q < 0 ? 0 : q > N - 1 ? N - 1 : q;
		*(float *)(dst + (long)y * dls + 4l * x) = (zero_fill && q != qc) ? 0.0f : s[qc];
	}
}

// op 0: x += a; 1: x *= a; 2: x += -v[y] (the median shift); 3: scale21 from the row's min and max, skip flag into info
__global__ __launch_bounds__(256) void k_elem_op(char *p, long sx, long sy, int w, int h, int op, float a, float b, const float *v, const float *v2, int *info)
{
	const int x = blockIdx.x * 256 + threadIdx.x;
	if (x >= w)
		return;
	for (int y = blockIdx.y; y < h; y += gridDim.y) {
		float *e = (float *)(p + (long)y * sx + (long)x * sy);
		if (op == 0)
			*e += a;
		else if (op == 1)
			*e *= a;
		else if (op == 2)
			*e += -v[y];
		else {
			const float mn = v[y], mx = v2[y];
			const bool skip = mx == mn;
			if (!skip)
				*e = (*e + scale_add(a, mn)) * scale_mul(a, b, mn, mx);
			if (info && x == 0)
				info[4 * y + 3] = skip;
		}
	}
}

__global__ __launch_bounds__(256) void k_info_init(int *info, int n_lines)
{
	const int y = blockIdx.x * 256 + threadIdx.x;
	if (y < n_lines) {
		info[4 * y] = 0;
		info[4 * y + 1] = 0;
		info[4 * y + 2] = -1;
		info[4 * y + 3] = 0;
	}
}

dim3 grid2(int w, int h) { return dim3((w + 255) / 256, h < 16384 ? h : 16384); } // (past the cap: tests/test_hip_grid_limits.py)

} // namespace

int cond_rows_per_group(int N)
{
	constexpr long budget = 152 * 1024; // of the CU's 160 KiB: the static arrays of the kernel take 6 KiB
	const long row = 4l * (((N + 3) & ~3) + 4);
	const long r = budget / row;
	return (int)(r > kCondMaxRows ? kCondMaxRows : r);
}

hipError_t launch_cond_lines(CondLineArgs a, hipStream_t s)
{
	if (a.n_lines <= 0)
		return hipSuccess;
	if (a.N < 1 || a.N > N1D_MAX)
		return hipErrorInvalidValue;
	a.rows = cond_rows_per_group(a.N);
	if (a.rows > a.n_lines)
		a.rows = a.n_lines;
	const size_t lds = (size_t)a.rows * 4 * (((a.N + 3) & ~3) + 4);
	hipError_t e = allow_lds((const void *)k_cond_lines, lds);
	if (e != hipSuccess)
		return e;
	k_cond_lines<<<(a.n_lines + a.rows - 1) / a.rows, 256, lds, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_rows_median(const char *p, long ls, int n_lines, int N, float *med, hipStream_t s)
{
	k_rows_median<<<n_lines, 256, 0, s>>>(p, ls, N, med);
	return hipGetLastError();
}

hipError_t launch_rows_minmax(const char *p, long ls, int n_lines, int N, float *mn, float *mx, hipStream_t s)
{
	k_rows_minmax<<<n_lines, 256, 0, s>>>(p, ls, N, mn, mx);
	return hipGetLastError();
}

hipError_t launch_rows_center(const char *p, long ls, int n_lines, int N, int *center, int *displ, int *info, int *moved, int *warn,
	int skip_done, hipStream_t s)
{
	k_rows_center<<<(n_lines + 63) / 64, 64, 0, s>>>(p, ls, n_lines, N, center, displ, info, moved, warn, skip_done);
	return hipGetLastError();
}

hipError_t launch_rows_displace(const char *src, long sls, char *dst, long dls, int n_lines, int N, const int *displ, int displ_all, int zero_fill, hipStream_t s)
{
	k_rows_displace<<<grid2(N, n_lines), 256, 0, s>>>(src, sls, dst, dls, n_lines, N, displ, displ_all, zero_fill);
	return hipGetLastError();
}

hipError_t launch_elem_op(char *p, long sx, long sy, int w, int h, int op, float a, float b, const float *v, const float *v2, int *info, hipStream_t s)
{
	k_elem_op<<<grid2(w, h), 256, 0, s>>>(p, sx, sy, w, h, op, a, b, v, v2, info);
	return hipGetLastError();
}

hipError_t launch_info_init(int *info, int n_lines, hipStream_t s)
{
	k_info_init<<<(n_lines + 255) / 256, 256, 0, s>>>(info, n_lines);
	return hipGetLastError();
}

} // namespace dwt
