// dwt_eaw97.hip -- the edge-avoiding CDF 9/7 wavelet ("WCDF 9/7") of libdwt on the device: dwt_eaw97_f_ex_stride_s /
// _i_ex_stride_s (src/eaw-experimental.c:73-186, 188-298).
//
// A pass computes one weight per sample pair from its own input,
//   w[i] = 1 / (|x[i] - x[i+1]|^alpha + 1e-5)   (i < N-1; w[N-1] = 0),
// and runs four lifting phases with those same weights: predict 1 on the odd samples, update 1 on the even ones,
// predict 2, update 2, each step  t[i] -+= (wL*t[l] + wR*t[r]) / (wL+wR) * (2*c)  -- minus in a predict, plus in an
// update, the product after the division -- then scales.  The reference's line ends are the same expression with
//   i == 0:    l = r = 1,    wL = wR = w[0]
//   i == N-1:  l = r = N-2,  wL = wR = w[N-2]      (an update when N is odd, a predict when N is even)
// so a phase is "every sample of one parity", and each phase reads only the other parity: it runs in place.  The
// inverse scales, then undoes update 2, predict 2, update 1, predict 1 with the signs swapped.  Nothing is fused or
// reordered and every division is IEEE, so a sample is the same function of the same inputs whichever kernel
// computes it.  Two routes share the step function, as for the 5/3 wavelet (dwt_eaw.hip):
//
//  * k_eaw97_line (+ k_eaw_place of dwt_eaw.hip): one exact pass over the lines of any strided frame, one thread per
//    sample pair, which holds the pair's window of 9 samples and 8 weights in registers and lifts it in place.
//  * k_eaw97_fwd_tile / k_eaw97_inv_tile: one launch per level of a dense Mallat frame.  A workgroup owns a 64 x 64
//    tile, reads it with its halo into LDS once, lifts rows and columns in place there (halo rows and columns
//    recomputed, never exchanged), and writes the subbands and both weight arrays of its own samples.
#include "dwt_eaw_steps.h"
#include "dwt_kernels.h"

#include <math.h>

namespace dwt {

// ---- the step (src/eaw-experimental.c:100-175, 219-294) -------------------------------------------------------------

// The constants of src/inline.h:310-315 as floats; k(s) is the reference's folded (2.f * c) of phase s.
struct Eaw97 {
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
};

// t[i] -= / += (wL * t[l] + wR * t[r]) / (wL + wR) * (2.f * c); a line end passes its one neighbour and weight twice
static __device__ __forceinline__ float eaw97_sub(float x, float a, float b, float wl, float wr, float k) { return x - (wl * a + wr * b) / (wl + wr) * k; }
static __device__ __forceinline__ float eaw97_add(float x, float a, float b, float wl, float wr, float k) { return x + (wl * a + wr * b) / (wl + wr) * k; }

// Phase s of a pass on sample i of a line of N >= 2 samples, T(i) the line's current values, Wt(i) its weights.
// Forward: s = 0 .. 3 are predict 1, update 1, predict 2, update 2 (odd, even, odd, even samples); inverse: update 2,
// predict 2, update 1, predict 1 undone (even, odd, even, odd).  Even phases subtract, odd phases add, both ways.
template <bool INV, class T, class Wt>
static __device__ __forceinline__ float eaw97_step(int s, const T &t, const Wt &w, int i, int N)
{
	const float k = Eaw97::k<INV>(s);
	int l = i - 1, r = i + 1, il = i - 1, ir = i;
	if (i == 0)
		l = 1, il = 0;
	else if (i == N - 1)
		r = N - 2, ir = N - 2;
	return (s & 1) ? eaw97_add(t(i), t(l), t(r), w(il), w(ir), k) : eaw97_sub(t(i), t(l), t(r), w(il), w(ir), k);
}

// ---- the exact line pass ---------------------------------------------------------------------------------------------

// Sample pair k of a line (samples 2k, 2k+1) is a function of 9 samples: forward 2k-4 .. 2k+4 (the even output needs
// update 2 <- predict 2 at +-1 <- update 1 at +-2 <- predict 1 at +-3 <- x at +-4, the odd one a sample less on each
// side), inverse 2k-3 .. 2k+5.  With the window at t[0 .. 8] (sample base + j at t[j]) both directions run phase s on
// the window's places j = 1+s, 3+s, .. <= 7-s, and the pair ends at t[4], t[5] (forward) or t[3], t[4] (inverse).
template <bool INV>
static __device__ __forceinline__ void eaw97_window(float (&t)[9], const float (&w)[8], int base, int N)
{
#pragma unroll
	for (int s = 0; s < 4; s++) {
		const float k = Eaw97::k<INV>(s);
#pragma unroll
		for (int j = 1 + s; j <= 7 - s; j += 2) {
			const int i = base + j;
			if (i < 0 || i >= N)
				continue;
			// the ends: i == 0 takes its right neighbour and w[0] twice, i == N-1 its left one and w[N-2]
			const float a = i == 0 ? t[j + 1] : t[j - 1], b = i == N - 1 ? t[j - 1] : t[j + 1];
			const float wl = i == 0 ? w[j] : w[j - 1], wr = i == N - 1 ? w[j - 1] : w[j];
			t[j] = (s & 1) ? eaw97_add(t[j], a, b, wl, wr, k) : eaw97_sub(t[j], a, b, wl, wr, k);
		}
	}
}

// n_lines lines, line l at src + l*ls, its elements es bytes apart.  Forward: reads samples 0..N-1 in order, writes the
// pass's result in sample order to tmp[l*N ..] and the weights to w[l*N ..].  Inverse: reads sample i at eaw_pos(i),
// weights from w, writes the line in order to tmp.  lanes_along_lines: neighbouring lanes take neighbouring lines
// (columns of a row-major image), otherwise neighbouring pairs of one line.
template <bool INV>
__global__ __launch_bounds__(256) void k_eaw97_line(const char *__restrict__ src, long ls, long es, int n_lines, int N, int hoff,
	float *__restrict__ tmp, float *__restrict__ w, int lanes_along_lines, float alpha, int mode)
{
	const int np = (N + 1) >> 1;
	const long total = (long)np * n_lines;
	for (long th = (long)blockIdx.x * blockDim.x + threadIdx.x; th < total; th += (long)gridDim.x * blockDim.x) {
		const int l = lanes_along_lines ? (int)(th % n_lines) : (int)(th / np);
		const int k = lanes_along_lines ? (int)(th / n_lines) : (int)(th % np);
		const char *line = src + (long)l * ls;
		float *out = tmp + (long)l * N;
		float *wl = w + (long)l * N;
		if (N == 1) { // scaled only; no weight written (src/eaw-experimental.c:87-92, 201-206)
			out[0] = *(const float *)line * (INV ? Eaw97::s2() : Eaw97::s1());
			continue;
		}
		float t[9], wt[8];
		const int base = INV ? 2 * k - 3 : 2 * k - 4;
#pragma unroll
		for (int j = 0; j < 9; j++) {
			const int i = base + j;
			t[j] = 0.f;
			if (i >= 0 && i < N) {
				if constexpr (INV)
					t[j] = *(const float *)(line + eaw_pos(i, hoff) * es) * ((i & 1) ? Eaw97::s1() : Eaw97::s2());
				else
					t[j] = *(const float *)(line + i * es);
			}
		}
#pragma unroll
		for (int j = 0; j < 8; j++) {
			const int i = base + j;
			wt[j] = 0.f;
			if (i >= 0 && i < N - 1)
				wt[j] = INV ? wl[i] : eaw_weight(t[j], t[j + 1], alpha, mode);
		}
		if constexpr (!INV) { // w[2k], w[2k+1] (0 at N-1) before the window is lifted
			wl[2 * k] = wt[4];
			if (2 * k + 1 < N)
				wl[2 * k + 1] = wt[5];
		}
		eaw97_window<INV>(t, wt, base, N);
		if constexpr (!INV) {
			out[2 * k] = t[4] * Eaw97::s1();
			if (2 * k + 1 < N)
				out[2 * k + 1] = t[5] * Eaw97::s2();
		} else {
			out[2 * k] = t[3];
			if (2 * k + 1 < N)
				out[2 * k + 1] = t[4];
		}
	}
}

hipError_t launch_eaw97_line(bool inverse, const void *src, long ls, long es, int n_lines, int N, int hoff, float *tmp, float *w,
	bool lanes_along_lines, float alpha, hipStream_t s)
{
	if (n_lines <= 0 || N <= 0)
		return hipSuccess;
	const dim3 grid = eaw_grid((long)((N + 1) >> 1) * n_lines);
	if (inverse)
		k_eaw97_line<true><<<grid, 256, 0, s>>>((const char *)src, ls, es, n_lines, N, hoff, tmp, w, lanes_along_lines, alpha, 1);
	else
		k_eaw97_line<false><<<grid, 256, 0, s>>>((const char *)src, ls, es, n_lines, N, hoff, tmp, w, lanes_along_lines, alpha, eaw_mode(alpha));
	return hipGetLastError();
}

// ---- one fused level of a dense Mallat frame -----------------------------------------------------------------------

// A workgroup owns samples [y0, y0+64) x [x0, x0+64) of the level's W x H input (forward) / output (inverse); x0 and
// y0 are even.  Halo, by dependency.  Forward: the odd output x0+63 needs update 1 at x0+64, that predict 1 at x0+65,
// that x[x0+66] and w[x0+65] = f(x[x0+65], x[x0+66]): 3 after; the even output x0 needs predict 2 at x0-1, update 1 at
// x0-2, predict 1 at x0-3, x[x0-4]: 4 before.  Inverse: the odd output x0+63 needs the even x0+64 with update 1
// undone, that the odd x0+65 with predict 2 undone, that the even x0+66 with update 2 undone, that the input at
// x0+67: 4 after; the even output x0 needs the odd x0-1 (predict 2 undone), that the even x0-2, that the input at
// x0-3: 3 before.  So both tiles are 71 x 71 samples, and phase s of a pass covers the samples of its parity in
// [lo + 1 + s, lo + 69 - s] (lo the tile's first halo sample), clipped to the frame, where the line-end forms apply.
constexpr int kEaw97T = 64;          // tile side
constexpr int kEaw97R = kEaw97T + 7; // tile + halo
// LDS row pitch, odd: a row phase puts neighbouring lanes on neighbouring rows (73 mod 64 = 9 is coprime to the 64
// banks), a column phase and the loads put them on neighbouring columns -- neither meets a bank conflict.
constexpr int kEaw97P = 73;

// Phase s of the pass along x (ROWS) or y of the LDS tile xs with weights ws, in place: samples of the phase's parity
// in [g0 + 1 + s, g0 + 69 - s] along the pass, lines [n0, n1) across it (LDS indices), neighbouring lanes on
// neighbouring lines.
template <bool INV, bool ROWS>
static __device__ __forceinline__ void eaw97_tile_phase(int s, float *xs, const float *ws, int g0, int N, int n0, int n1, int g_across0,
	int N_across, int tid)
{
	// g0 + 1 + s has the phase's parity: g0 is even in the forward tile and odd in the inverse one
	const int first = g0 + 1 + s, cnt = (kEaw97R - 2 - 2 * s + 1) / 2, nl = n1 - n0;
	for (int e = tid; e < cnt * nl; e += 256) {
		const int n = n0 + e % nl, g = first + 2 * (e / nl);
		const int ga = g_across0 + n;
		if (g < 0 || g >= N || ga < 0 || ga >= N_across)
			continue;
		const int c = g - g0;
		if (ROWS) {
			float *xr = xs + n * kEaw97P;
			const float *wr = ws + n * kEaw97P;
			xr[c] = eaw97_step<INV>(s, [&](int i) { return xr[i - g0]; }, [&](int i) { return wr[i - g0]; }, g, N);
		} else {
			float *xc = xs + n;
			const float *wc = ws + n;
			xc[c * kEaw97P] = eaw97_step<INV>(s, [&](int i) { return xc[(i - g0) * kEaw97P]; }, [&](int i) { return wc[(i - g0) * kEaw97P]; }, g, N);
		}
	}
}

// Forward: in (W x H, pitch pin floats) -> LL to ll (pitch pll), HL / LH / HH to det at their Mallat offsets (pitch pd);
// wH (H x W, row-major) and wV (W x H, column-major).  Images of a batch are bi_* floats apart.
__global__ __launch_bounds__(256) void k_eaw97_fwd_tile(const float *__restrict__ in, long pin, long bi_in, float *__restrict__ ll, long pll,
	long bi_ll, float *__restrict__ det, long pd, long bi_det, float *__restrict__ wH, float *__restrict__ wV, long bi_w, int W, int H,
	float alpha, int mode)
{
	__shared__ float xs[kEaw97R * kEaw97P]; // input; the row pass in place; the column pass in place
	__shared__ float ws[kEaw97R * kEaw97P]; // row weights, then column weights
	const int tid = threadIdx.x;
	const int x0 = blockIdx.x * kEaw97T, y0 = blockIdx.y * kEaw97T;
	const int b = blockIdx.z;
	in += b * bi_in;
	ll += b * bi_ll;
	det += b * bi_det;
	wH += b * bi_w;
	wV += b * bi_w;
	const int gx0 = x0 - 4, gy0 = y0 - 4; // LDS (r, c) holds sample (gy0 + r, gx0 + c)
	const int ye = min(y0 + kEaw97T, H), xe = min(x0 + kEaw97T, W);
	const int Wd = (W + 1) >> 1, Hd = (H + 1) >> 1;

	// 1. input with halo (only samples inside the frame; the steps never read others)
	for (int e = tid; e < kEaw97R * kEaw97R; e += 256) {
		const int r = e / kEaw97R, c = e % kEaw97R, gy = gy0 + r, gx = gx0 + c;
		if (gy >= 0 && gy < H && gx >= 0 && gx < W)
			xs[r * kEaw97P + c] = in[gy * pin + gx];
	}
	__syncthreads();
	// 2. row weights w[gx] = f(x[gx], x[gx+1]) for gx in [x0-4, x0+66); the tile's own rows and columns go to wH
	for (int e = tid; e < kEaw97R * (kEaw97R - 1); e += 256) {
		const int r = e / (kEaw97R - 1), c = e % (kEaw97R - 1), gy = gy0 + r, gx = gx0 + c;
		if (gy < 0 || gy >= H || gx < 0 || gx >= W)
			continue;
		const float v = gx < W - 1 ? eaw_weight(xs[r * kEaw97P + c], xs[r * kEaw97P + c + 1], alpha, mode) : 0.f;
		ws[r * kEaw97P + c] = v;
		if (gy >= y0 && gy < ye && gx >= x0 && gx < xe)
			wH[(long)gy * W + gx] = v;
	}
	__syncthreads();
	// 3. rows: predict 1, update 1, predict 2, update 2 over every row of the tile and its halo, in place
	for (int s = 0; s < 4; s++) {
		eaw97_tile_phase<false, true>(s, xs, ws, gx0, W, 0, kEaw97R, gy0, H, tid);
		__syncthreads();
	}
	// 4. the row pass's scaling of the tile's columns (even * s1, odd * s2)
	for (int e = tid; e < kEaw97R * kEaw97T; e += 256) {
		const int r = e / kEaw97T, c = 4 + e % kEaw97T, gy = gy0 + r, gx = gx0 + c;
		if (gy >= 0 && gy < H && gx < W)
			xs[r * kEaw97P + c] = xs[r * kEaw97P + c] * ((gx & 1) ? Eaw97::s2() : Eaw97::s1());
	}
	__syncthreads();
	// 5. column weights over rows gy in [y0-4, y0+66) of the tile's columns (the row weights are no longer read)
	for (int e = tid; e < (kEaw97R - 1) * kEaw97T; e += 256) {
		const int r = e / kEaw97T, c = 4 + e % kEaw97T, gy = gy0 + r, gx = gx0 + c;
		if (gy < 0 || gy >= H || gx >= W)
			continue;
		ws[r * kEaw97P + c] = gy < H - 1 ? eaw_weight(xs[r * kEaw97P + c], xs[(r + 1) * kEaw97P + c], alpha, mode) : 0.f;
	}
	__syncthreads();
	// wV of the tile's own columns: column gx is a run of H floats; lanes along y through the LDS copy
	for (int e = tid; e < kEaw97T * kEaw97T; e += 256) {
		const int cc = e / kEaw97T, ry = e % kEaw97T, gy = y0 + ry, gx = x0 + cc;
		if (gy < ye && gx < xe) // column gx sits at its Mallat place after the row pass
			wV[(long)((gx & 1) ? Wd + (gx >> 1) : (gx >> 1)) * H + gy] = ws[(ry + 4) * kEaw97P + cc + 4];
	}
	// 6. columns: predict 1, update 1, predict 2 in place; update 2 goes straight out
	for (int s = 0; s < 3; s++) {
		eaw97_tile_phase<false, false>(s, xs, ws, gy0, H, 4, 4 + kEaw97T, gx0, W, tid);
		__syncthreads();
	}
	// 7. column update 2 of even gy in [y0, y0+64), scaling, and the four subbands' stores (lanes along x)
	for (int e = tid; e < (kEaw97T / 2) * kEaw97T; e += 256) {
		const int c = 4 + e % kEaw97T, gy = y0 + 2 * (e / kEaw97T), gx = gx0 + c, r = gy - gy0;
		if (gy >= H || gx >= W)
			continue;
		const float *xc = xs + c, *wc = ws + c;
		const float v = eaw97_step<false>(3, [&](int i) { return xc[(i - gy0) * kEaw97P]; }, [&](int i) { return wc[(i - gy0) * kEaw97P]; }, gy, H) *
		                Eaw97::s1();
		const int ox = (gx & 1) ? Wd + (gx >> 1) : (gx >> 1), oy = gy >> 1;
		if (gx & 1)
			det[(long)oy * pd + ox] = v;
		else
			ll[(long)oy * pll + ox] = v;
		if (gy + 1 < H)
			det[(long)(Hd + oy) * pd + ox] = xs[(r + 1) * kEaw97P + c] * Eaw97::s2();
	}
}

// Inverse: the level's subbands -- LL from ll (pitch pll), HL / LH / HH from det at their Mallat offsets (pitch pd) --
// and its weights wH (H x W, row-major), wV (W x H, column-major) -> the W x H result to out (pitch pout).
__global__ __launch_bounds__(256) void k_eaw97_inv_tile(const float *__restrict__ ll, long pll, long bi_ll, const float *__restrict__ det,
	long pd, long bi_det, const float *__restrict__ wH, const float *__restrict__ wV, long bi_w, float *__restrict__ out, long pout,
	long bi_out, int W, int H)
{
	__shared__ float xs[kEaw97R * kEaw97P]; // column pass input (scaled), lifted in place; then the row pass in place
	__shared__ float wv[kEaw97R * kEaw97P]; // column weights (r, c) = wV[gx][gy]; then the row weights
	const int tid = threadIdx.x;
	const int x0 = blockIdx.x * kEaw97T, y0 = blockIdx.y * kEaw97T;
	const int b = blockIdx.z;
	ll += b * bi_ll;
	det += b * bi_det;
	wH += b * bi_w;
	wV += b * bi_w;
	out += b * bi_out;
	const int gx0 = x0 - 3, gy0 = y0 - 3; // LDS (r, c) holds sample (gy0 + r, gx0 + c)
	const int Wd = (W + 1) >> 1, Hd = (H + 1) >> 1;

	// 1. input with halo, at its Mallat place, scaled as the column pass scales it (even rows * s2, odd * s1)
	for (int e = tid; e < kEaw97R * kEaw97R; e += 256) {
		const int r = e / kEaw97R, c = e % kEaw97R, gy = gy0 + r, gx = gx0 + c;
		if (gy < 0 || gy >= H || gx < 0 || gx >= W)
			continue;
		const int oy = (gy & 1) ? Hd + (gy >> 1) : (gy >> 1), ox = (gx & 1) ? Wd + (gx >> 1) : (gx >> 1);
		const float v = ((gx | gy) & 1) ? det[(long)oy * pd + ox] : ll[(long)oy * pll + ox];
		xs[r * kEaw97P + c] = v * ((gy & 1) ? Eaw97::s1() : Eaw97::s2());
	}
	// column weights gy in [y0-3, y0+67): lanes along y (wV is column-major)
	for (int e = tid; e < kEaw97R * (kEaw97R - 1); e += 256) {
		const int c = e / (kEaw97R - 1), r = e % (kEaw97R - 1), gy = gy0 + r, gx = gx0 + c;
		if (gy >= 0 && gy < H - 1 && gx >= 0 && gx < W)
			wv[r * kEaw97P + c] = wV[(long)((gx & 1) ? Wd + (gx >> 1) : (gx >> 1)) * H + gy];
	}
	__syncthreads();
	// 2. columns: update 2, predict 2, update 1, predict 1 undone over every column of the tile and its halo, in place
	for (int s = 0; s < 4; s++) {
		eaw97_tile_phase<true, false>(s, xs, wv, gy0, H, 0, kEaw97R, gx0, W, tid);
		__syncthreads();
	}
	// 3. the row pass's scaling of the tile's rows (even * s2, odd * s1), and their weights gx in [x0-3, x0+67)
	for (int e = tid; e < kEaw97T * kEaw97R; e += 256) {
		const int r = 3 + e / kEaw97R, c = e % kEaw97R, gy = gy0 + r, gx = gx0 + c;
		if (gy < H && gx >= 0 && gx < W)
			xs[r * kEaw97P + c] = xs[r * kEaw97P + c] * ((gx & 1) ? Eaw97::s1() : Eaw97::s2());
	}
	for (int e = tid; e < kEaw97T * (kEaw97R - 1); e += 256) {
		const int r = 3 + e / (kEaw97R - 1), c = e % (kEaw97R - 1), gy = gy0 + r, gx = gx0 + c;
		if (gy < H && gx >= 0 && gx < W - 1)
			wv[r * kEaw97P + c] = wH[(long)gy * W + gx];
	}
	__syncthreads();
	// 4. rows: update 2, predict 2, update 1 undone in place; predict 1 is undone on the way out
	for (int s = 0; s < 3; s++) {
		eaw97_tile_phase<true, true>(s, xs, wv, gx0, W, 3, 3 + kEaw97T, gy0, H, tid);
		__syncthreads();
	}
	// 5. rows: predict 1 undone at odd gx, and the tile's stores (lanes along x)
	for (int e = tid; e < kEaw97T * kEaw97T; e += 256) {
		const int r = 3 + e / kEaw97T, gx = x0 + e % kEaw97T, gy = gy0 + r;
		if (gy >= H || gx >= W)
			continue;
		const float *xr = xs + r * kEaw97P, *wr = wv + r * kEaw97P;
		float v = xr[gx - gx0];
		if (gx & 1)
			v = eaw97_step<true>(3, [&](int i) { return xr[i - gx0]; }, [&](int i) { return wr[i - gx0]; }, gx, W);
		out[(long)gy * pout + gx] = v;
	}
}

hipError_t launch_eaw97_level(bool inverse, const EawLevelArgs &a, float alpha, hipStream_t s)
{
	if (a.W < 2 || a.H < 2 || a.batch <= 0)
		return hipErrorInvalidValue;
	const dim3 grid((a.W + kEaw97T - 1) / kEaw97T, (a.H + kEaw97T - 1) / kEaw97T, a.batch);
	if (inverse)
		k_eaw97_inv_tile<<<grid, 256, 0, s>>>(a.ll, a.pll, a.bi_ll, a.det, a.pd, a.bi_det, a.wH, a.wV, a.bi_w, a.out, a.pout, a.bi_out, a.W, a.H);
	else
		k_eaw97_fwd_tile<<<grid, 256, 0, s>>>(a.in, a.pin, a.bi_in, a.ll_out, a.pll, a.bi_ll, a.det_out, a.pd, a.bi_det, a.wH_out, a.wV_out,
			a.bi_w, a.W, a.H, alpha, eaw_mode(alpha));
	return hipGetLastError();
}

} // namespace dwt
