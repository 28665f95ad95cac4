// dwt_eaw.hip -- the edge-avoiding wavelets (EAW, Fattal 2009) of libdwt on the device: CDF 5/3, dwt_eaw53_f_ex_stride_s /
// _i_ex_stride_s and their in-place twins (src/libdwt.c:11070-11240, 11868-12000), and CDF 9/7 ("WCDF 9/7"),
// dwt_eaw97_f_ex_stride_s / _i_ex_stride_s (src/eaw-experimental.c:73-186, 188-298).
//
// A pass computes one weight per sample pair from its own input,
//   w[i] = 1 / (|x[i] - x[i+1]|^alpha + 1e-5)   (i < N-1; w[N-1] = 0),
// and runs K lifting phases with those same weights (5/3: predict, update; 9/7: predict 1, update 1, predict 2,
// update 2), a predict on the odd samples and an update on the even ones, each step
//   t[i] -+= (wL*t[l] + wR*t[r]) / (a function of wL+wR)
// -- minus in a predict, plus in an update -- then scales.  The reference's line ends are the same expression with
//   i == 0:    l = r = 1,    wL = wR = w[0]
//   i == N-1:  l = r = N-2,  wL = wR = w[N-2]      (an update when N is odd, a predict when N is even)
// so a phase is "every sample of one parity", and each phase reads only the other parity: it runs in place.  The
// inverse scales, then undoes the phases last to first with the signs swapped.  What a wavelet is -- K, the two scale
// factors and the expression of one step, written exactly as the reference writes it -- is its policy (Eaw53, Eaw97);
// everything else is one set of templates over the policy.  Nothing is fused or reordered and every division is IEEE,
// so a sample is the same function of the same inputs whichever kernel computes it.  Two routes share the policies:
//
//  * k_eaw_line (+ k_eaw_place): one exact pass over the lines of any strided frame, one thread per sample pair,
//    which holds the pair's window of 2K+1 samples and 2K weights in registers and lifts it in place; results go to a
//    dense scratch, then to their places.  Sparse frames, zero padding, the interleaved layout and option
//    "eaw_two_pass" run here.
//  * k_eaw_fwd_tile / k_eaw_inv_tile: one launch per level of a dense Mallat frame.  A workgroup owns a 64 x 64 tile,
//    reads it with its halo into LDS once, lifts rows and columns in place there (halo rows and columns recomputed,
//    never exchanged), and writes the subbands and both weight arrays of its own samples.
#include "dwt_kernels.h"

#include <math.h>

namespace dwt {

// ---- what the wavelets share -----------------------------------------------------------------------------------------

// dwt_eaw_w (src/libdwt.c:11070, src/eaw-experimental.c:56).  mode 0: alpha == 0 (powf(x, 0) == 1 for every x); mode 1:
// alpha == 1 (powf(x, 1) == x for every float); mode 2: any other alpha, pow in double rounded once to float (within
// 1 ulp of glibc's powf).
static __device__ __forceinline__ float eaw_weight(float n, float m, float alpha, int mode)
{
	const float eps = 1.0e-5f;
	const float d = fabsf(n - m);
	float p;
	if (mode == 0)
		p = 1.f;
	else if (mode == 1)
		p = d;
	else
		p = (float)pow((double)d, (double)alpha);
	return 1.f / (p + eps);
}

// Where sample i of a line sits: Mallat (L at i/2, H at hoff + i/2) or interleaved (at i).
static __device__ __forceinline__ long eaw_pos(int i, int hoff) { return hoff < 0 ? i : (i & 1) ? hoff + (i >> 1) : (i >> 1); }

static inline int eaw_mode(float alpha) { return alpha == 0.f ? 0 : alpha == 1.f ? 1 : 2; }

static inline dim3 eaw_grid(long threads)
{
	long b = (threads + 255) / 256;
	return dim3((unsigned)(b < 65536 ? (b > 0 ? b : 1) : 65536)); // (past the cap: tests/test_hip_grid_limits.py)
}

// ---- the two wavelets ------------------------------------------------------------------------------------------------

// step<INV>(s, x, a, b, wl, wr): phase s of a pass on a sample x with its neighbours a, b and their weights.  Forward:
// s = 0 .. K-1 are predict, update, .. (odd, even, .. samples); inverse: the last update undone, the last predict, ..
// (even, odd, ..).  Even phases subtract, odd phases add, both ways.

// src/libdwt.c:11070-11240, 11868-11939
struct Eaw53 {
	static constexpr int kPhases = 2;
	static __device__ __forceinline__ float s1() { return 1.41421356237309504880f; } // dwt_cdf53_s1_s (src/inline.h:334)
	static __device__ __forceinline__ float s2() { return 0.70710678118654752440f; } // dwt_cdf53_s2_s
	template <bool INV>
	static __device__ __forceinline__ float step(int s, float x, float a, float b, float wl, float wr)
	{
		if (INV ? s == 0 : s == 1) { // the update and its inverse
			const float u = (wl * a + wr * b) / (2.f * (wl + wr));
			return INV ? x - u : x + u;
		}
		const float p = (wl * a + wr * b) / (wl + wr);
		return INV ? x + p : x - p;
	}
};

// src/eaw-experimental.c:100-175, 219-294; the constants of src/inline.h:310-315 as floats, k(s) the reference's folded
// (2.f * c) of phase s, the product after the division
struct Eaw97 {
	static constexpr int kPhases = 4;
	static __device__ __forceinline__ float s1() { return 1.1496043988602f; }
	static __device__ __forceinline__ float s2() { return (float)(1 / 1.1496043988602); }
	template <bool INV>
	static __device__ __forceinline__ float k(int s)
	{
		const float p1 = 2.f * 1.58613434342059f, u1 = 2.f * -0.0529801185729f, p2 = 2.f * -0.8829110755309f, u2 = 2.f * 0.4435068520439f;
		if (INV)
			return s == 0 ? u2 : s == 1 ? p2 : s == 2 ? u1 : p1;
		return s == 0 ? p1 : s == 1 ? u1 : s == 2 ? p2 : u2;
	}
	template <bool INV>
	static __device__ __forceinline__ float step(int s, float x, float a, float b, float wl, float wr)
	{
		const float q = (wl * a + wr * b) / (wl + wr) * k<INV>(s);
		return (s & 1) ? x + q : x - q;
	}
};

// Phase s on sample i of a line of N >= 2 samples, T(i) the line's current values, Wt(i) its weights: a line end
// passes its one neighbour and that neighbour's weight twice.
template <class P, bool INV, class T, class Wt>
static __device__ __forceinline__ float eaw_step(int s, const T &t, const Wt &w, int i, int N)
{
	int l = i - 1, r = i + 1, il = i - 1, ir = i;
	if (i == 0)
		l = 1, il = 0;
	else if (i == N - 1)
		r = N - 2, ir = N - 2;
	return P::template step<INV>(s, t(i), t(l), t(r), w(il), w(ir));
}

// ---- the exact line pass ---------------------------------------------------------------------------------------------

// Sample pair k of a line (samples 2k, 2k+1) is a function of 2K+1 samples: forward 2k-K .. 2k+K (the even output
// needs the last update <- a predict at +-1 <- an update at +-2 <- .. <- x at +-K, the odd one a sample less on each
// side), inverse 2k-K+1 .. 2k+K+1.  With the window at t[0 .. 2K] (sample base + j at t[j]) both directions run phase
// s on the window's places j = 1+s, 3+s, .. <= 2K-1-s, and the pair ends at t[K], t[K+1] (forward) or t[K-1], t[K]
// (inverse).
template <class P, bool INV>
static __device__ __forceinline__ void eaw_window(float (&t)[2 * P::kPhases + 1], const float (&w)[2 * P::kPhases], int base, int N)
{
	constexpr int K = P::kPhases;
#pragma unroll
	for (int s = 0; s < K; s++) {
#pragma unroll
		for (int j = 1 + s; j <= 2 * K - 1 - s; j += 2) {
			const int i = base + j;
			if (i < 0 || i >= N)
				continue;
			// the ends: i == 0 takes its right neighbour and w[0] twice, i == N-1 its left one and w[N-2]
			const float a = i == 0 ? t[j + 1] : t[j - 1], b = i == N - 1 ? t[j - 1] : t[j + 1];
			const float wl = i == 0 ? w[j] : w[j - 1], wr = i == N - 1 ? w[j - 1] : w[j];
			t[j] = P::template step<INV>(s, t[j], a, b, wl, wr);
		}
	}
}

// n_lines lines, line l at src + l*ls, its elements es bytes apart.  Forward: reads samples 0..N-1 in order, writes the
// pass's result in sample order to tmp[l*N ..] and the weights to w[l*N ..].  Inverse: reads sample i at eaw_pos(i),
// weights from w, writes the line in order to tmp.  lanes_along_lines: neighbouring lanes take neighbouring lines
// (columns of a row-major image), otherwise neighbouring pairs of one line.
template <class P, bool INV>
__global__ __launch_bounds__(256) void k_eaw_line(const char *__restrict__ src, long ls, long es, int n_lines, int N, int hoff,
	float *__restrict__ tmp, float *__restrict__ w, int lanes_along_lines, float alpha, int mode)
{
	constexpr int K = P::kPhases;
	const int np = (N + 1) >> 1;
	const long total = (long)np * n_lines;
	for (long th = (long)blockIdx.x * blockDim.x + threadIdx.x; th < total; th += (long)gridDim.x * blockDim.x) {
		const int l = lanes_along_lines ? (int)(th % n_lines) : (int)(th / np);
		const int k = lanes_along_lines ? (int)(th / n_lines) : (int)(th % np);
		const char *line = src + (long)l * ls;
		float *out = tmp + (long)l * N;
		float *wl = w + (long)l * N;
		if (N == 1) { // scaled only; no weight written (src/libdwt.c:11118-11123, 11878-11883; src/eaw-experimental.c:87-92, 201-206)
			out[0] = *(const float *)line * (INV ? P::s2() : P::s1());
			continue;
		}
		float t[2 * K + 1], wt[2 * K];
		const int base = INV ? 2 * k - K + 1 : 2 * k - K;
#pragma unroll
		for (int j = 0; j < 2 * K + 1; j++) {
			const int i = base + j;
			t[j] = 0.f;
			if (i >= 0 && i < N) {
				if constexpr (INV)
					t[j] = *(const float *)(line + eaw_pos(i, hoff) * es) * ((i & 1) ? P::s1() : P::s2());
				else
					t[j] = *(const float *)(line + i * es);
			}
		}
#pragma unroll
		for (int j = 0; j < 2 * K; j++) {
			const int i = base + j;
			wt[j] = 0.f;
			if (i >= 0 && i < N - 1)
				wt[j] = INV ? wl[i] : eaw_weight(t[j], t[j + 1], alpha, mode);
		}
		if constexpr (!INV) { // w[2k], w[2k+1] (0 at N-1) before the window is lifted
			wl[2 * k] = wt[K];
			if (2 * k + 1 < N)
				wl[2 * k + 1] = wt[K + 1];
		}
		eaw_window<P, INV>(t, wt, base, N);
		if constexpr (!INV) {
			out[2 * k] = t[K] * P::s1();
			if (2 * k + 1 < N)
				out[2 * k + 1] = t[K + 1] * P::s2();
		} else {
			out[2 * k] = t[K - 1];
			if (2 * k + 1 < N)
				out[2 * k + 1] = t[K];
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

template <class P>
static hipError_t eaw_line(bool inverse, const void *src, long ls, long es, int n_lines, int N, int hoff, float *tmp, float *w,
	bool lanes_along_lines, float alpha, hipStream_t s)
{
	const dim3 grid = eaw_grid((long)((N + 1) >> 1) * n_lines);
	if (inverse)
		k_eaw_line<P, true><<<grid, 256, 0, s>>>((const char *)src, ls, es, n_lines, N, hoff, tmp, w, lanes_along_lines, alpha, 1);
	else
		k_eaw_line<P, false><<<grid, 256, 0, s>>>((const char *)src, ls, es, n_lines, N, hoff, tmp, w, lanes_along_lines, alpha, eaw_mode(alpha));
	return hipGetLastError();
}

hipError_t launch_eaw_line(EawWavelet wv, bool inverse, const void *src, long ls, long es, int n_lines, int N, int hoff, float *tmp,
	float *w, bool lanes_along_lines, float alpha, hipStream_t s)
{
	if (n_lines <= 0 || N <= 0)
		return hipSuccess;
	return wv == kEaw97 ? eaw_line<Eaw97>(inverse, src, ls, es, n_lines, N, hoff, tmp, w, lanes_along_lines, alpha, s)
	                    : eaw_line<Eaw53>(inverse, src, ls, es, n_lines, N, hoff, tmp, w, lanes_along_lines, alpha, s);
}

hipError_t launch_eaw_place(void *dst, long ls, long es, int n_lines, int N, int hoff, const float *tmp, bool lanes_along_lines, hipStream_t s)
{
	if (n_lines <= 0 || N <= 0)
		return hipSuccess;
	k_eaw_place<<<eaw_grid((long)N * n_lines), 256, 0, s>>>((char *)dst, ls, es, n_lines, N, hoff, tmp, lanes_along_lines);
	return hipGetLastError();
}

// ---- one fused level of a dense Mallat frame -----------------------------------------------------------------------

// A workgroup owns samples [y0, y0+64) x [x0, x0+64) of the level's W x H input (forward) / output (inverse); x0 and
// y0 are even.  Halo, by dependency (9/7, K = 4).  Forward: the odd output x0+63 needs update 1 at x0+64, that predict
// 1 at x0+65, that x[x0+66] and w[x0+65] = f(x[x0+65], x[x0+66]): K-1 after; the even output x0 needs predict 2 at
// x0-1, update 1 at x0-2, predict 1 at x0-3, x[x0-4]: K before.  Inverse: the odd output x0+63 needs the even x0+64
// with update 1 undone, that the odd x0+65 with predict 2 undone, that the even x0+66 with update 2 undone, that the
// input at x0+67: K after; the even output x0 needs the odd x0-1 (predict 2 undone), that the even x0-2, that the
// input at x0-3: K-1 before.  The same chains, two links shorter, give 5/3 (K = 2) 2 and 1.  So both tiles are R x R
// samples, R = 64 + 2K - 1 (5/3: 67, 9/7: 71), and phase s of a pass covers the samples of its parity in
// [lo + 1 + s, lo + R - 2 - s] (lo the tile's first halo sample), clipped to the frame, where the line-end forms apply.
constexpr int kEawT = 64; // tile side
template <class P>
constexpr int kEawR = kEawT + 2 * P::kPhases - 1; // tile + halo
// LDS row pitch, odd (5/3: 69, 9/7: 73): a row phase puts neighbouring lanes on neighbouring rows (an odd pitch is
// coprime to the 64 banks), a column phase and the loads put them on neighbouring columns -- neither meets a bank
// conflict.
template <class P>
constexpr int kEawP = (kEawR<P> + 1) | 1;

// Phase s of the pass along x (ROWS) or y of the LDS tile xs with weights ws, in place: samples of the phase's parity
// in [g0 + 1 + s, g0 + R - 2 - s] along the pass, lines [n0, n1) across it (LDS indices), neighbouring lanes on
// neighbouring lines.
template <class P, bool INV, bool ROWS>
static __device__ __forceinline__ void eaw_tile_phase(int s, float *xs, const float *ws, int g0, int N, int n0, int n1, int g_across0,
	int N_across, int tid)
{
	constexpr int R = kEawR<P>, Pt = kEawP<P>;
	// g0 + 1 + s has the phase's parity: K is even, so g0 is even in the forward tile and odd in the inverse one
	static_assert(P::kPhases % 2 == 0);
	const int first = g0 + 1 + s, cnt = (R - 2 - 2 * s + 1) / 2, nl = n1 - n0;
	for (int e = tid; e < cnt * nl; e += 256) {
		const int n = n0 + e % nl, g = first + 2 * (e / nl);
		const int ga = g_across0 + n;
		if (g < 0 || g >= N || ga < 0 || ga >= N_across)
			continue;
		const int c = g - g0;
		if (ROWS) {
			float *xr = xs + n * Pt;
			const float *wr = ws + n * Pt;
			xr[c] = eaw_step<P, INV>(s, [&](int i) { return xr[i - g0]; }, [&](int i) { return wr[i - g0]; }, g, N);
		} else {
			float *xc = xs + n;
			const float *wc = ws + n;
			xc[c * Pt] = eaw_step<P, INV>(s, [&](int i) { return xc[(i - g0) * Pt]; }, [&](int i) { return wc[(i - g0) * Pt]; }, g, N);
		}
	}
}

// Forward: in (W x H, pitch pin floats) -> LL to ll (pitch pll), HL / LH / HH to det at their Mallat offsets (pitch pd);
// wH (H x W, row-major) and wV (W x H, column-major).  Images of a batch are bi_* floats apart.
template <class P>
__global__ __launch_bounds__(256) void k_eaw_fwd_tile(const float *__restrict__ in, long pin, long bi_in, float *__restrict__ ll, long pll,
	long bi_ll, float *__restrict__ det, long pd, long bi_det, float *__restrict__ wH, float *__restrict__ wV, long bi_w, int W, int H,
	float alpha, int mode)
{
	constexpr int K = P::kPhases, T = kEawT, R = kEawR<P>, Pt = kEawP<P>;
	__shared__ float xs[R * Pt]; // input; the row pass in place; the column pass in place
	__shared__ float ws[R * Pt]; // row weights, then column weights
	const int tid = threadIdx.x;
	const int x0 = blockIdx.x * T, y0 = blockIdx.y * T;
	const int b = blockIdx.z;
	in += b * bi_in;
	ll += b * bi_ll;
	det += b * bi_det;
	wH += b * bi_w;
	wV += b * bi_w;
	const int gx0 = x0 - K, gy0 = y0 - K; // LDS (r, c) holds sample (gy0 + r, gx0 + c)
	const int ye = min(y0 + T, H), xe = min(x0 + T, W);
	const int Wd = (W + 1) >> 1, Hd = (H + 1) >> 1;

	// 1. input with halo (only samples inside the frame; the steps never read others)
	for (int e = tid; e < R * R; e += 256) {
		const int r = e / R, c = e % R, gy = gy0 + r, gx = gx0 + c;
		if (gy >= 0 && gy < H && gx >= 0 && gx < W)
			xs[r * Pt + c] = in[gy * pin + gx];
	}
	__syncthreads();
	// 2. row weights w[gx] = f(x[gx], x[gx+1]) for gx in [x0-K, x0+62+K); the tile's own rows and columns go to wH
	for (int e = tid; e < R * (R - 1); e += 256) {
		const int r = e / (R - 1), c = e % (R - 1), gy = gy0 + r, gx = gx0 + c;
		if (gy < 0 || gy >= H || gx < 0 || gx >= W)
			continue;
		const float v = gx < W - 1 ? eaw_weight(xs[r * Pt + c], xs[r * Pt + c + 1], alpha, mode) : 0.f;
		ws[r * Pt + c] = v;
		if (gy >= y0 && gy < ye && gx >= x0 && gx < xe)
			wH[(long)gy * W + gx] = v;
	}
	__syncthreads();
	// 3. rows: every phase over every row of the tile and its halo, in place
	for (int s = 0; s < K; s++) {
		eaw_tile_phase<P, false, true>(s, xs, ws, gx0, W, 0, R, gy0, H, tid);
		__syncthreads();
	}
	// 4. the row pass's scaling of the tile's columns (even * s1, odd * s2)
	for (int e = tid; e < R * T; e += 256) {
		const int r = e / T, c = K + e % T, gy = gy0 + r, gx = gx0 + c;
		if (gy >= 0 && gy < H && gx < W)
			xs[r * Pt + c] = xs[r * Pt + c] * ((gx & 1) ? P::s2() : P::s1());
	}
	__syncthreads();
	// 5. column weights over rows gy in [y0-K, y0+62+K) of the tile's columns (the row weights are no longer read)
	for (int e = tid; e < (R - 1) * T; e += 256) {
		const int r = e / T, c = K + e % T, gy = gy0 + r, gx = gx0 + c;
		if (gy < 0 || gy >= H || gx >= W)
			continue;
		ws[r * Pt + c] = gy < H - 1 ? eaw_weight(xs[r * Pt + c], xs[(r + 1) * Pt + c], alpha, mode) : 0.f;
	}
	__syncthreads();
	// wV of the tile's own columns: column gx is a run of H floats; lanes along y through the LDS copy
	for (int e = tid; e < T * T; e += 256) {
		const int cc = e / T, ry = e % T, gy = y0 + ry, gx = x0 + cc;
		if (gy < ye && gx < xe) // column gx sits at its Mallat place after the row pass
			wV[(long)((gx & 1) ? Wd + (gx >> 1) : (gx >> 1)) * H + gy] = ws[(ry + K) * Pt + cc + K];
	}
	// 6. columns: every phase but the last in place; the last update goes straight out
	for (int s = 0; s < K - 1; s++) {
		eaw_tile_phase<P, false, false>(s, xs, ws, gy0, H, K, K + T, gx0, W, tid);
		__syncthreads();
	}
	// 7. the columns' last update of even gy in [y0, y0+64), scaling, and the four subbands' stores (lanes along x)
	for (int e = tid; e < (T / 2) * T; e += 256) {
		const int c = K + e % T, gy = y0 + 2 * (e / T), gx = gx0 + c, r = gy - gy0;
		if (gy >= H || gx >= W)
			continue;
		const float *xc = xs + c, *wc = ws + c;
		const float v = eaw_step<P, false>(K - 1, [&](int i) { return xc[(i - gy0) * Pt]; }, [&](int i) { return wc[(i - gy0) * Pt]; }, gy, H) *
		                P::s1();
		const int ox = (gx & 1) ? Wd + (gx >> 1) : (gx >> 1), oy = gy >> 1;
		if (gx & 1)
			det[(long)oy * pd + ox] = v;
		else
			ll[(long)oy * pll + ox] = v;
		if (gy + 1 < H)
			det[(long)(Hd + oy) * pd + ox] = xs[(r + 1) * Pt + c] * P::s2();
	}
}

// Inverse: the level's subbands -- LL from ll (pitch pll), HL / LH / HH from det at their Mallat offsets (pitch pd) --
// and its weights wH (H x W, row-major), wV (W x H, column-major) -> the W x H result to out (pitch pout).
template <class P>
__global__ __launch_bounds__(256) void k_eaw_inv_tile(const float *__restrict__ ll, long pll, long bi_ll, const float *__restrict__ det,
	long pd, long bi_det, const float *__restrict__ wH, const float *__restrict__ wV, long bi_w, float *__restrict__ out, long pout,
	long bi_out, int W, int H)
{
	constexpr int K = P::kPhases, T = kEawT, R = kEawR<P>, Pt = kEawP<P>;
	__shared__ float xs[R * Pt]; // column pass input (scaled), lifted in place; then the row pass in place
	__shared__ float wv[R * Pt]; // column weights (r, c) = wV[gx][gy]; then the row weights
	const int tid = threadIdx.x;
	const int x0 = blockIdx.x * T, y0 = blockIdx.y * T;
	const int b = blockIdx.z;
	ll += b * bi_ll;
	det += b * bi_det;
	wH += b * bi_w;
	wV += b * bi_w;
	out += b * bi_out;
	const int gx0 = x0 - (K - 1), gy0 = y0 - (K - 1); // LDS (r, c) holds sample (gy0 + r, gx0 + c)
	const int Wd = (W + 1) >> 1, Hd = (H + 1) >> 1;

	// 1. input with halo, at its Mallat place, scaled as the column pass scales it (even rows * s2, odd * s1)
	for (int e = tid; e < R * R; e += 256) {
		const int r = e / R, c = e % R, gy = gy0 + r, gx = gx0 + c;
		if (gy < 0 || gy >= H || gx < 0 || gx >= W)
			continue;
		const int oy = (gy & 1) ? Hd + (gy >> 1) : (gy >> 1), ox = (gx & 1) ? Wd + (gx >> 1) : (gx >> 1);
		const float v = ((gx | gy) & 1) ? det[(long)oy * pd + ox] : ll[(long)oy * pll + ox];
		xs[r * Pt + c] = v * ((gy & 1) ? P::s1() : P::s2());
	}
	// column weights gy in [y0-K+1, y0+63+K): lanes along y (wV is column-major)
	for (int e = tid; e < R * (R - 1); e += 256) {
		const int c = e / (R - 1), r = e % (R - 1), gy = gy0 + r, gx = gx0 + c;
		if (gy >= 0 && gy < H - 1 && gx >= 0 && gx < W)
			wv[r * Pt + c] = wV[(long)((gx & 1) ? Wd + (gx >> 1) : (gx >> 1)) * H + gy];
	}
	__syncthreads();
	// 2. columns: every phase undone over every column of the tile and its halo, in place
	for (int s = 0; s < K; s++) {
		eaw_tile_phase<P, true, false>(s, xs, wv, gy0, H, 0, R, gx0, W, tid);
		__syncthreads();
	}
	// 3. the row pass's scaling of the tile's rows (even * s2, odd * s1), and their weights gx in [x0-K+1, x0+63+K)
	for (int e = tid; e < T * R; e += 256) {
		const int r = K - 1 + e / R, c = e % R, gy = gy0 + r, gx = gx0 + c;
		if (gy < H && gx >= 0 && gx < W)
			xs[r * Pt + c] = xs[r * Pt + c] * ((gx & 1) ? P::s1() : P::s2());
	}
	for (int e = tid; e < T * (R - 1); e += 256) {
		const int r = K - 1 + e / (R - 1), c = e % (R - 1), gy = gy0 + r, gx = gx0 + c;
		if (gy < H && gx >= 0 && gx < W - 1)
			wv[r * Pt + c] = wH[(long)gy * W + gx];
	}
	__syncthreads();
	// 4. rows: every phase but the last undone in place; the first predict is undone on the way out
	for (int s = 0; s < K - 1; s++) {
		eaw_tile_phase<P, true, true>(s, xs, wv, gx0, W, K - 1, K - 1 + T, gy0, H, tid);
		__syncthreads();
	}
	// 5. rows: the first predict undone at odd gx, and the tile's stores (lanes along x)
	for (int e = tid; e < T * T; e += 256) {
		const int r = K - 1 + e / T, gx = x0 + e % T, gy = gy0 + r;
		if (gy >= H || gx >= W)
			continue;
		const float *xr = xs + r * Pt, *wr = wv + r * Pt;
		float v = xr[gx - gx0];
		if (gx & 1)
			v = eaw_step<P, true>(K - 1, [&](int i) { return xr[i - gx0]; }, [&](int i) { return wr[i - gx0]; }, gx, W);
		out[(long)gy * pout + gx] = v;
	}
}

template <class P>
static hipError_t eaw_level(bool inverse, const EawLevelArgs &a, float alpha, hipStream_t s)
{
	const dim3 grid((a.W + kEawT - 1) / kEawT, (a.H + kEawT - 1) / kEawT, a.batch);
	if (inverse)
		k_eaw_inv_tile<P><<<grid, 256, 0, s>>>(a.ll, a.pll, a.bi_ll, a.det, a.pd, a.bi_det, a.wH, a.wV, a.bi_w, a.out, a.pout, a.bi_out, a.W, a.H);
	else
		k_eaw_fwd_tile<P><<<grid, 256, 0, s>>>(a.in, a.pin, a.bi_in, a.ll_out, a.pll, a.bi_ll, a.det_out, a.pd, a.bi_det, a.wH_out, a.wV_out,
			a.bi_w, a.W, a.H, alpha, eaw_mode(alpha));
	return hipGetLastError();
}

hipError_t launch_eaw_level(EawWavelet wv, bool inverse, const EawLevelArgs &a, float alpha, hipStream_t s)
{
	if (a.W < 2 || a.H < 2 || a.batch <= 0)
		return hipErrorInvalidValue;
	return wv == kEaw97 ? eaw_level<Eaw97>(inverse, a, alpha, s) : eaw_level<Eaw53>(inverse, a, alpha, s);
}

} // namespace dwt
