// dwt_eaw.hip -- the edge-avoiding CDF 5/3 wavelets (EAW, Fattal 2009) of libdwt on the device:
// dwt_eaw53_f_ex_stride_s / _i_ex_stride_s and their in-place twins (src/libdwt.c:11070-11240, 11868-12000).
//
// Every pass first computes a weight per sample pair from its own input,
//   w[i] = 1 / (|x[i] - x[i+1]|^alpha + 1e-5)   (i < N-1; w[N-1] = 0),
// then predicts the odd samples and updates the even ones with them, each step divided by the sum of its weights, and
// scales.  Each step is written here exactly as the reference writes it -- the line ends keep their literal
// (wL*a + wR*a) / (...) forms, nothing is fused or reordered, every division is IEEE -- so a sample is the same
// function of the same inputs on both sides, whichever kernel computes it.  Two routes share those step functions:
//
//  * k_eaw_line (+ k_eaw_place): one exact pass over the lines of any strided frame, one thread per sample pair, the
//    pair's neighbourhood recomputed from global memory; results go to a dense scratch, then to their places.  Sparse
//    frames, zero padding, the interleaved layout and option "eaw_two_pass" run here.
//  * k_eaw_fwd_tile / k_eaw_inv_tile: one launch per level of a dense Mallat frame.  A workgroup owns a 64 x 64 tile,
//    reads it with its halo into LDS once, lifts the rows it needs (halo rows recomputed, never exchanged), then the
//    columns, and writes the subbands and both weight arrays of its own samples.
#include "dwt_eaw_steps.h"
#include "dwt_kernels.h"

#include <math.h>

namespace dwt {

// ---- the steps (src/libdwt.c:11070-11240, 11868-11939) --------------------------------------------------------------

struct Eaw53 {
	static __device__ __forceinline__ float s1() { return 1.41421356237309504880f; } // dwt_cdf53_s1_s (src/inline.h:334)
	static __device__ __forceinline__ float s2() { return 0.70710678118654752440f; } // dwt_cdf53_s2_s
};

// forward predict of an odd sample with both neighbours / at the end of an even line (wL = wR = w[N-2])
static __device__ __forceinline__ float f_pred(float x, float xl, float xr, float wl, float wr) { return x - (wl * xl + wr * xr) / (wl + wr); }
static __device__ __forceinline__ float f_pred_end(float x, float xl, float w) { return x - (w * xl + w * xl) / (w + w); }
// forward update of an even sample with both neighbours / at a line end (first sample; last of an odd line)
static __device__ __forceinline__ float f_upd(float x, float dl, float dr, float wl, float wr) { return x + (wl * dl + wr * dr) / (2.f * (wl + wr)); }
static __device__ __forceinline__ float f_upd_end(float x, float d, float w) { return x + (w * d + w * d) / (2.f * (w + w)); }
// inverse: the update undone, then the predict
static __device__ __forceinline__ float i_upd(float x, float dl, float dr, float wl, float wr) { return x - (wl * dl + wr * dr) / (2.f * (wl + wr)); }
static __device__ __forceinline__ float i_upd_end(float x, float d, float w) { return x - (w * d + w * d) / (2.f * (w + w)); }
static __device__ __forceinline__ float i_pred(float x, float el, float er, float wl, float wr) { return x + (wl * el + wr * er) / (wl + wr); }
static __device__ __forceinline__ float i_pred_end(float x, float el, float w) { return x + (w * el + w * el) / (w + w); }

// ---- one sample pair of a line, from an accessor (N >= 2) ------------------------------------------------------------

// Forward: X(i) the line's input.  Pair k: even sample 2k -> *lo (scaled), odd 2k+1 -> *hi (if 2k+1 < N), weights
// w[2k], w[2k+1] -> *w0, *w1 (0 past N-2).
template <class X>
static __device__ __forceinline__ void fwd_pair(const X &x, int N, int k, float alpha, int mode, float *lo, float *hi, float *w0, float *w1)
{
	auto W = [&](int i) { return eaw_weight(x(i), x(i + 1), alpha, mode); };
	// predicted odd sample i (unscaled)
	auto D = [&](int i) {
		const float wl = W(i - 1);
		if (i + 1 < N)
			return f_pred(x(i), x(i - 1), x(i + 1), wl, W(i));
		return f_pred_end(x(i), x(i - 1), wl); // i == N-1, N even
	};
	const int i = 2 * k;
	const float wi = i < N - 1 ? W(i) : 0.f;
	float s;
	if (i == 0)
		s = f_upd_end(x(0), D(1), wi);
	else if (i == N - 1) // N odd
		s = f_upd_end(x(i), D(i - 1), W(i - 1));
	else
		s = f_upd(x(i), D(i - 1), D(i + 1), W(i - 1), wi);
	*lo = s * Eaw53::s1();
	*w0 = wi;
	if (i + 1 < N) {
		*hi = D(i + 1) * Eaw53::s2();
		*w1 = i + 1 < N - 1 ? W(i + 1) : 0.f;
	}
}

// Inverse: T(i) the line's input already scaled (even * s2, odd * s1), Wt(i) the weights.  Pair k: samples 2k, 2k+1.
template <class T, class Wt>
static __device__ __forceinline__ void inv_pair(const T &t, const Wt &W, int N, int k, float *e0, float *o1)
{
	// even sample i with the update undone
	auto E = [&](int i) {
		if (i == 0)
			return i_upd_end(t(0), t(1), W(0));
		if (i == N - 1) // N odd
			return i_upd_end(t(i), t(i - 1), W(i - 1));
		return i_upd(t(i), t(i - 1), t(i + 1), W(i - 1), W(i));
	};
	const int i = 2 * k;
	const float e = E(i);
	*e0 = e;
	if (i + 1 < N) {
		const int o = i + 1;
		if (o + 1 < N)
			*o1 = i_pred(t(o), e, E(o + 1), W(o - 1), W(o));
		else
			*o1 = i_pred_end(t(o), e, W(o - 1)); // N even
	}
}

// ---- the exact line pass ---------------------------------------------------------------------------------------------

// n_lines lines, line l at src + l*ls, its elements es bytes apart.  Forward: reads samples 0..N-1 in order, writes the
// pass's result in sample order to tmp[l*N ..] and the weights to w[l*N ..].  Inverse: reads sample i at eaw_pos(i),
// weights from w, writes the line in order to tmp.  lanes_along_lines: neighbouring lanes take neighbouring lines
// (columns of a row-major image), otherwise neighbouring pairs of one line.
template <bool INV>
__global__ __launch_bounds__(256) void k_eaw_line(const char *__restrict__ src, long ls, long es, int n_lines, int N, int hoff,
	float *__restrict__ tmp, float *__restrict__ w, int lanes_along_lines, float alpha, int mode)
{
	const int np = (N + 1) >> 1;
	const long total = (long)np * n_lines;
	for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
		const int l = lanes_along_lines ? (int)(t % n_lines) : (int)(t / np);
		const int k = lanes_along_lines ? (int)(t / n_lines) : (int)(t % np);
		const char *line = src + (long)l * ls;
		float *out = tmp + (long)l * N;
		float *wl = w + (long)l * N;
		if (N == 1) { // scaled only; no weight written (src/libdwt.c:11118-11123, 11878-11883)
			out[0] = *(const float *)line * (INV ? Eaw53::s2() : Eaw53::s1());
			continue;
		}
		if constexpr (!INV) {
			auto x = [&](int i) { return *(const float *)(line + i * es); };
			float lo, hi, w0, w1;
			fwd_pair(x, N, k, alpha, mode, &lo, &hi, &w0, &w1);
			out[2 * k] = lo;
			wl[2 * k] = w0;
			if (2 * k + 1 < N) {
				out[2 * k + 1] = hi;
				wl[2 * k + 1] = w1;
			}
		} else {
			auto tt = [&](int i) { return *(const float *)(line + eaw_pos(i, hoff) * es) * ((i & 1) ? Eaw53::s1() : Eaw53::s2()); };
			auto W = [&](int i) { return wl[i]; };
			float e0, o1;
			inv_pair(tt, W, N, k, &e0, &o1);
			out[2 * k] = e0;
			if (2 * k + 1 < N)
				out[2 * k + 1] = o1;
		}
	}
}

// tmp (n_lines x N, sample order) to the lines: sample i to eaw_pos(i, hoff) (forward) or i (inverse: hoff = -1)
__global__ __launch_bounds__(256) void k_eaw_place(char *__restrict__ dst, long ls, long es, int n_lines, int N, int hoff,
	const float *__restrict__ tmp, int lanes_along_lines)
{
	const long total = (long)N * n_lines;
	for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
		const int l = lanes_along_lines ? (int)(t % n_lines) : (int)(t / N);
		const int i = lanes_along_lines ? (int)(t / n_lines) : (int)(t % N);
		*(float *)(dst + (long)l * ls + eaw_pos(i, hoff) * es) = tmp[(long)l * N + i];
	}
}

hipError_t launch_eaw_line(bool inverse, const void *src, long ls, long es, int n_lines, int N, int hoff, float *tmp, float *w,
	bool lanes_along_lines, float alpha, hipStream_t s)
{
	if (n_lines <= 0 || N <= 0)
		return hipSuccess;
	const dim3 grid = eaw_grid((long)((N + 1) >> 1) * n_lines);
	if (inverse)
		k_eaw_line<true><<<grid, 256, 0, s>>>((const char *)src, ls, es, n_lines, N, hoff, tmp, w, lanes_along_lines, alpha, 1);
	else
		k_eaw_line<false><<<grid, 256, 0, s>>>((const char *)src, ls, es, n_lines, N, hoff, tmp, w, lanes_along_lines, alpha, eaw_mode(alpha));
	return hipGetLastError();
}

hipError_t launch_eaw_place(void *dst, long ls, long es, int n_lines, int N, int hoff, const float *tmp, bool lanes_along_lines, hipStream_t s)
{
	if (n_lines <= 0 || N <= 0)
		return hipSuccess;
	k_eaw_place<<<eaw_grid((long)N * n_lines), 256, 0, s>>>((char *)dst, ls, es, n_lines, N, hoff, tmp, lanes_along_lines);
	return hipGetLastError();
}

// ---- one fused level of a dense Mallat frame -----------------------------------------------------------------------

// A workgroup owns samples [y0, y0+64) x [x0, x0+64) of the level's W x H input (forward) / output (inverse).
constexpr int kEawT = 64;      // tile side
constexpr int kEawR = kEawT + 3; // tile + halo: forward 2 before, 1 after; inverse 1 before, 2 after
constexpr int kEawP = kEawR + 1; // LDS row pitch

// Forward: in (W x H, pitch pin floats) -> LL to ll (pitch pll), HL / LH / HH to det at their Mallat offsets (pitch pd);
// wH (H x W, row-major) and wV (W x H, column-major).  Images of a batch are bi_* floats apart.
__global__ __launch_bounds__(256) void k_eaw_fwd_tile(const float *__restrict__ in, long pin, long bi_in, float *__restrict__ ll, long pll,
	long bi_ll, float *__restrict__ det, long pd, long bi_det, float *__restrict__ wH, float *__restrict__ wV, long bi_w, int W, int H,
	float alpha, int mode)
{
	__shared__ float xs[kEawR * kEawP]; // input, then the row weights' scratch of the column pass
	__shared__ float ws[kEawR * kEawP]; // row weights, then column weights
	__shared__ float rt[kEawR * kEawP]; // the row-lifted tile (sample order), then the column pass in place
	const int tid = threadIdx.x;
	const int x0 = blockIdx.x * kEawT, y0 = blockIdx.y * kEawT;
	const int b = blockIdx.z;
	in += b * bi_in;
	ll += b * bi_ll;
	det += b * bi_det;
	wH += b * bi_w;
	wV += b * bi_w;
	const int gx0 = x0 - 2, gy0 = y0 - 2; // LDS (r, c) holds sample (gy0 + r, gx0 + c)
	const int ye = min(y0 + kEawT, H), xe = min(x0 + kEawT, W);
	const int Wd = (W + 1) >> 1, Hd = (H + 1) >> 1;

	// 1. input with halo (only samples inside the frame; the steps never read others)
	for (int e = tid; e < kEawR * kEawR; e += 256) {
		const int r = e / kEawR, c = e % kEawR, gy = gy0 + r, gx = gx0 + c;
		if (gy >= 0 && gy < H && gx >= 0 && gx < W)
			xs[r * kEawP + c] = in[gy * pin + gx];
	}
	__syncthreads();
	// 2. row weights w[gx] = f(x[gx], x[gx+1]) for gx in [x0-2, x0+64); the tile's own rows and columns go to wH
	for (int e = tid; e < kEawR * (kEawT + 2); e += 256) {
		const int r = e / (kEawT + 2), c = e % (kEawT + 2), gy = gy0 + r, gx = gx0 + c;
		if (gy < 0 || gy >= H || gx < 0 || gx >= W)
			continue;
		const float v = gx < W - 1 ? eaw_weight(xs[r * kEawP + c], xs[r * kEawP + c + 1], alpha, mode) : 0.f;
		ws[r * kEawP + c] = v;
		if (gy >= y0 && gy < ye && gx >= x0)
			wH[(long)gy * W + gx] = v;
	}
	__syncthreads();
	// 3. row predict: odd gx in [x0-1, x0+64), unscaled, in place (reads even samples only)
	for (int e = tid; e < kEawR * (kEawT / 2 + 1); e += 256) {
		const int r = e / (kEawT / 2 + 1), gx = x0 - 1 + 2 * (e % (kEawT / 2 + 1)), gy = gy0 + r, c = gx - gx0;
		if (gy < 0 || gy >= H || gx < 0 || gx >= W)
			continue;
		const float *xr = xs + r * kEawP;
		const float v = gx + 1 < W ? f_pred(xr[c], xr[c - 1], xr[c + 1], ws[r * kEawP + c - 1], ws[r * kEawP + c])
		                           : f_pred_end(xr[c], xr[c - 1], ws[r * kEawP + c - 1]);
		xs[r * kEawP + c] = v;
	}
	__syncthreads();
	// 4. row update of even gx in [x0, x0+64) and scaling -> rt (tile columns, sample order)
	for (int e = tid; e < kEawR * (kEawT / 2); e += 256) {
		const int r = e / (kEawT / 2), gx = x0 + 2 * (e % (kEawT / 2)), gy = gy0 + r, c = gx - gx0;
		if (gy < 0 || gy >= H || gx >= W)
			continue;
		const float *xr = xs + r * kEawP, *wr = ws + r * kEawP;
		float s;
		if (gx == 0)
			s = f_upd_end(xr[c], xr[c + 1], wr[c]);
		else if (gx == W - 1)
			s = f_upd_end(xr[c], xr[c - 1], wr[c - 1]);
		else
			s = f_upd(xr[c], xr[c - 1], xr[c + 1], wr[c - 1], wr[c]);
		rt[r * kEawP + (c - 2)] = s * Eaw53::s1();
		if (gx + 1 < W)
			rt[r * kEawP + (c - 1)] = xr[c + 1] * Eaw53::s2();
	}
	__syncthreads();
	// 5. column weights over rows gy in [y0-2, y0+64): ws[r][cc] = f(rt[r][cc], rt[r+1][cc])
	for (int e = tid; e < (kEawT + 2) * kEawT; e += 256) {
		const int r = e / kEawT, cc = e % kEawT, gy = gy0 + r, gx = x0 + cc;
		if (gy < 0 || gy >= H || gx >= W)
			continue;
		ws[r * kEawP + cc] = gy < H - 1 ? eaw_weight(rt[r * kEawP + cc], rt[(r + 1) * kEawP + cc], alpha, mode) : 0.f;
	}
	__syncthreads();
	// wV of the tile's own columns: column gx is a run of H floats; lanes along y through the LDS copy
	for (int e = tid; e < kEawT * kEawT; e += 256) {
		const int cc = e / kEawT, ry = e % kEawT, gy = y0 + ry, gx = x0 + cc;
		if (gy < ye && gx < xe) // column gx sits at its Mallat place after the row pass
			wV[(long)((gx & 1) ? Wd + (gx >> 1) : (gx >> 1)) * H + gy] = ws[(ry + 2) * kEawP + cc];
	}
	// 6. column predict: odd gy in [y0-1, y0+64) -> xs (scratch; rt's even rows are still read)
	for (int e = tid; e < (kEawT / 2 + 1) * kEawT; e += 256) {
		const int cc = e % kEawT, gy = y0 - 1 + 2 * (e / kEawT), gx = x0 + cc, r = gy - gy0;
		if (gy < 0 || gy >= H || gx >= W)
			continue;
		const float v = gy + 1 < H
			? f_pred(rt[r * kEawP + cc], rt[(r - 1) * kEawP + cc], rt[(r + 1) * kEawP + cc], ws[(r - 1) * kEawP + cc], ws[r * kEawP + cc])
			: f_pred_end(rt[r * kEawP + cc], rt[(r - 1) * kEawP + cc], ws[(r - 1) * kEawP + cc]);
		xs[r * kEawP + cc] = v;
	}
	__syncthreads();
	// 7. column update of even gy in [y0, y0+64), scaling, and the four subbands' stores (lanes along x)
	for (int e = tid; e < (kEawT / 2) * kEawT; e += 256) {
		const int cc = e % kEawT, gy = y0 + 2 * (e / kEawT), gx = x0 + cc, r = gy - gy0;
		if (gy >= H || gx >= W)
			continue;
		const float *wc = ws + cc;
		const float x = rt[r * kEawP + cc];
		float s;
		if (gy == 0)
			s = f_upd_end(x, xs[(r + 1) * kEawP + cc], wc[r * kEawP]);
		else if (gy == H - 1)
			s = f_upd_end(x, xs[(r - 1) * kEawP + cc], wc[(r - 1) * kEawP]);
		else
			s = f_upd(x, xs[(r - 1) * kEawP + cc], xs[(r + 1) * kEawP + cc], wc[(r - 1) * kEawP], wc[r * kEawP]);
		s = s * Eaw53::s1();
		const int ox = (gx & 1) ? Wd + (gx >> 1) : (gx >> 1), oy = gy >> 1;
		if (gx & 1)
			det[(long)oy * pd + ox] = s;
		else
			ll[(long)oy * pll + ox] = s;
		if (gy + 1 < H)
			det[(long)(Hd + oy) * pd + ox] = xs[(r + 1) * kEawP + cc] * Eaw53::s2();
	}
}

// Inverse: the level's subbands -- LL from ll (pitch pll), HL / LH / HH from det at their Mallat offsets (pitch pd) --
// and its weights wH (H x W, row-major), wV (W x H, column-major) -> the W x H result to out (pitch pout).
__global__ __launch_bounds__(256) void k_eaw_inv_tile(const float *__restrict__ ll, long pll, long bi_ll, const float *__restrict__ det,
	long pd, long bi_det, const float *__restrict__ wH, const float *__restrict__ wV, long bi_w, float *__restrict__ out, long pout,
	long bi_out, int W, int H)
{
	__shared__ float xs[kEawR * kEawP]; // column pass input (scaled), lifted in place; then the row pass in place
	__shared__ float wv[kEawR * kEawP]; // column weights (r, c) = wV[gx][gy]; then the row weights
	const int tid = threadIdx.x;
	const int x0 = blockIdx.x * kEawT, y0 = blockIdx.y * kEawT;
	const int b = blockIdx.z;
	ll += b * bi_ll;
	det += b * bi_det;
	wH += b * bi_w;
	wV += b * bi_w;
	out += b * bi_out;
	const int gx0 = x0 - 1, gy0 = y0 - 1; // LDS (r, c) holds sample (gy0 + r, gx0 + c)
	const int Wd = (W + 1) >> 1, Hd = (H + 1) >> 1;

	// 1. input with halo, at its Mallat place, scaled as the column pass scales it (even rows * s2, odd * s1)
	for (int e = tid; e < kEawR * kEawR; e += 256) {
		const int r = e / kEawR, c = e % kEawR, gy = gy0 + r, gx = gx0 + c;
		if (gy < 0 || gy >= H || gx < 0 || gx >= W)
			continue;
		const int oy = (gy & 1) ? Hd + (gy >> 1) : (gy >> 1), ox = (gx & 1) ? Wd + (gx >> 1) : (gx >> 1);
		const float v = ((gx | gy) & 1) ? det[(long)oy * pd + ox] : ll[(long)oy * pll + ox];
		xs[r * kEawP + c] = v * ((gy & 1) ? Eaw53::s1() : Eaw53::s2());
	}
	// column weights gy in [y0-1, y0+65): lanes along y (wV is column-major)
	for (int e = tid; e < kEawR * (kEawT + 2); e += 256) {
		const int c = e / (kEawT + 2), r = e % (kEawT + 2), gy = gy0 + r, gx = gx0 + c;
		if (gy >= 0 && gy < H - 1 && gx >= 0 && gx < W)
			wv[r * kEawP + c] = wV[(long)((gx & 1) ? Wd + (gx >> 1) : (gx >> 1)) * H + gy];
	}
	__syncthreads();
	// 2. columns: the update undone at even gy in [y0, y0+64] (reads odd rows only), in place
	for (int e = tid; e < (kEawT / 2 + 1) * kEawR; e += 256) {
		const int c = e % kEawR, gy = y0 + 2 * (e / kEawR), gx = gx0 + c, r = gy - gy0;
		if (gy >= H || gx < 0 || gx >= W)
			continue;
		const float *xc = xs + c, *wc = wv + c;
		float v;
		if (gy == 0)
			v = i_upd_end(xc[r * kEawP], xc[(r + 1) * kEawP], wc[r * kEawP]);
		else if (gy == H - 1)
			v = i_upd_end(xc[r * kEawP], xc[(r - 1) * kEawP], wc[(r - 1) * kEawP]);
		else
			v = i_upd(xc[r * kEawP], xc[(r - 1) * kEawP], xc[(r + 1) * kEawP], wc[(r - 1) * kEawP], wc[r * kEawP]);
		xs[r * kEawP + c] = v;
	}
	__syncthreads();
	// 3. columns: the predict undone at odd gy in [y0+1, y0+64), in place, then the row pass's scaling of the tile's rows
	for (int e = tid; e < (kEawT / 2) * kEawR; e += 256) {
		const int c = e % kEawR, gy = y0 + 1 + 2 * (e / kEawR), gx = gx0 + c, r = gy - gy0;
		if (gy >= H || gx < 0 || gx >= W)
			continue;
		const float *xc = xs + c, *wc = wv + c;
		const float v = gy + 1 < H
			? i_pred(xc[r * kEawP], xc[(r - 1) * kEawP], xc[(r + 1) * kEawP], wc[(r - 1) * kEawP], wc[r * kEawP])
			: i_pred_end(xc[r * kEawP], xc[(r - 1) * kEawP], wc[(r - 1) * kEawP]);
		xs[r * kEawP + c] = v;
	}
	__syncthreads();
	for (int e = tid; e < kEawT * kEawR; e += 256) {
		const int r = 1 + e / kEawR, c = e % kEawR, gy = gy0 + r, gx = gx0 + c;
		if (gy < H && gx >= 0 && gx < W)
			xs[r * kEawP + c] = xs[r * kEawP + c] * ((gx & 1) ? Eaw53::s1() : Eaw53::s2());
	}
	// row weights gx in [x0-1, x0+65) of the tile's rows (wv's column weights are no longer read)
	for (int e = tid; e < kEawT * (kEawT + 2); e += 256) {
		const int r = 1 + e / (kEawT + 2), c = e % (kEawT + 2), gy = gy0 + r, gx = gx0 + c;
		if (gy < H && gx >= 0 && gx < W - 1)
			wv[r * kEawP + c] = wH[(long)gy * W + gx];
	}
	__syncthreads();
	// 4. rows: the update undone at even gx in [x0, x0+64]
	for (int e = tid; e < kEawT * (kEawT / 2 + 1); e += 256) {
		const int r = 1 + e / (kEawT / 2 + 1), gx = x0 + 2 * (e % (kEawT / 2 + 1)), gy = gy0 + r, c = gx - gx0;
		if (gy >= H || gx >= W)
			continue;
		const float *xr = xs + r * kEawP, *wr = wv + r * kEawP;
		float v;
		if (gx == 0)
			v = i_upd_end(xr[c], xr[c + 1], wr[c]);
		else if (gx == W - 1)
			v = i_upd_end(xr[c], xr[c - 1], wr[c - 1]);
		else
			v = i_upd(xr[c], xr[c - 1], xr[c + 1], wr[c - 1], wr[c]);
		xs[r * kEawP + c] = v;
	}
	__syncthreads();
	// 5. rows: the predict undone at odd gx, and the tile's stores (lanes along x)
	for (int e = tid; e < kEawT * kEawT; e += 256) {
		const int r = 1 + e / kEawT, gx = x0 + e % kEawT, gy = gy0 + r, c = gx - gx0;
		if (gy >= H || gx >= W)
			continue;
		const float *xr = xs + r * kEawP, *wr = wv + r * kEawP;
		float v = xr[c];
		if (gx & 1)
			v = gx + 1 < W ? i_pred(v, xr[c - 1], xr[c + 1], wr[c - 1], wr[c]) : i_pred_end(v, xr[c - 1], wr[c - 1]);
		out[(long)gy * pout + gx] = v;
	}
}

hipError_t launch_eaw_level(bool inverse, const EawLevelArgs &a, float alpha, hipStream_t s)
{
	if (a.W < 2 || a.H < 2 || a.batch <= 0)
		return hipErrorInvalidValue;
	const dim3 grid((a.W + kEawT - 1) / kEawT, (a.H + kEawT - 1) / kEawT, a.batch);
	if (inverse)
		k_eaw_inv_tile<<<grid, 256, 0, s>>>(a.ll, a.pll, a.bi_ll, a.det, a.pd, a.bi_det, a.wH, a.wV, a.bi_w, a.out, a.pout, a.bi_out, a.W, a.H);
	else
		k_eaw_fwd_tile<<<grid, 256, 0, s>>>(a.in, a.pin, a.bi_in, a.ll_out, a.pll, a.bi_ll, a.det_out, a.pd, a.bi_det, a.wH_out, a.wV_out,
			a.bi_w, a.W, a.H, alpha, eaw_mode(alpha));
	return hipGetLastError();
}

} // namespace dwt
