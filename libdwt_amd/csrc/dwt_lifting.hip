// dwt_lifting.hip -- user-defined lifting wavelets on the device (include/libdwt_hip.h): a lifting scheme
// that arrives as a table in the kernel arguments, binary32 or wrapping int32.
//
// A step updates the samples of one parity of a line from up to four terms over samples of the other parity, so it runs
// in place; every tap reflects its INDEX into the line (whole-sample symmetric, multi-bounce) and reads the sample it
// lands on.  lift_eval is that step on one sample, written once: both routes call it, so a sample is the same function
// of the same inputs whichever kernel computes it.  Nothing is contracted (-ffp-contract=off) or reordered.
//
//  * k_lift_tile: one launch per level of dense frames.  A workgroup owns a 64 x 64 tile of the level, stages it with a
//    halo of R samples (the scheme's reach, <= 8) in LDS, runs the first pass over every line of that region and the
//    second over the tile's own lines, in place, and writes the four subbands (forward) or the tile (inverse).  The halo
//    is recomputed, never exchanged.  A step of reach r shrinks the span of correct samples by r on each side that lies
//    inside the frame; a side at or beyond the frame's border does not shrink, because there every tap reflects to a
//    sample of the span itself.  Positions outside the frame are never staged and never lifted: a halo filled by
//    reflection and lifted like interior samples is right only for symmetric steps.
//  * k_lift_step and its companions: the step-by-step route on a dense copy of the level, one elementwise launch per step
//    and direction.  The cross-check, and the route of schemes whose reach exceeds 8.
//  * k_lift_lines: every level of a batch of LINES of up to N1D_MAX samples in one launch, the line whole in LDS as two
//    parity arrays: no halo, so any reach.  k_lift_line_move gathers and places the lines of the
//    step-by-step route.
#include "dwt_kernels.h"
#include "dwt_line_lds.h"

#include <type_traits>

namespace dwt {

namespace {

constexpr int kT = LIFT_TILE;
constexpr int kSmax = kT + 2 * LIFT_FUSED_REACH; // the largest staged region's side
// LDS row pitch, odd: a row pass puts neighbouring lanes on neighbouring rows (an odd pitch is coprime to the 64 banks),
// a column pass and the loads put them on neighbouring columns
constexpr int kPt = kSmax + 1;
static_assert(kPt % 2 == 1, "odd LDS pitch");

// whole-sample symmetric reflection of index i into [0, N), N >= 2
static __device__ __forceinline__ int lift_reflect(int i, int N)
{
	while ((unsigned)i >= (unsigned)N)
		i = i < 0 ? -i : 2 * (N - 1) - i;
	return i;
}

// Step st on sample g of a line of N >= 2 samples whose current values are at(index): the new value of the sample.
// REFLECT false: the caller knows that every tap of g lies inside the line.
template <class T, bool INV, bool REFLECT = true, class At>
static __device__ __forceinline__ T lift_eval(const LiftStep &st, int g, int N, const At &at)
{
	auto tap = [&](int i) { return REFLECT ? lift_reflect(i, N) : i; };
	const T x = at(g);
	if constexpr (std::is_same<T, float>::value) {
		float sum = 0.f;
		for (int k = 0; k < st.n_terms; k++) {
			float a = at(tap(g + st.off_a[k]));
			if (st.off_b[k] != 0)
				a = a + at(tap(g + st.off_b[k]));
			const float t = st.coef[k] * a;
			sum = k == 0 ? t : sum + t;
		}
		return INV ? x - sum : x + sum;
	} else {
		unsigned acc = 0;
		for (int k = 0; k < st.n_terms; k++) {
			unsigned a = (unsigned)at(tap(g + st.off_a[k]));
			if (st.off_b[k] != 0)
				a += (unsigned)at(tap(g + st.off_b[k]));
			acc += (unsigned)st.num[k] * a;
		}
		const int v = (int)(acc + (unsigned)st.add) >> st.shift;
		const unsigned d = (st.sign > 0) != INV ? (unsigned)v : 0u - (unsigned)v;
		return (T)((unsigned)x + d);
	}
}

template <class T>
static __device__ __forceinline__ T lift_scaled(T v, float f)
{
	if constexpr (std::is_same<T, float>::value)
		return f != 1.0f ? v * f : v;
	else
		return v;
}

// where sample i of a line of N sits in the Mallat layout: L at i/2, H at ceil(N/2) + i/2
static __device__ __forceinline__ int lift_pos(int i, int N) { return (i & 1) ? ((N + 1) >> 1) + (i >> 1) : (i >> 1); }

// ---- the fused level ---------------------------------------------------------------------------------------------------

// f(n, k) for every line n in [n0, n1) and every k in [0, cnt), neighbouring lanes on neighbouring lines: runs of 64 lines
// take four k at a time, what is left of at most 16 lines sixteen -- no division by a run-time count.  n0, n1 and cnt are
// uniform.
template <class F>
static __device__ __forceinline__ void lift_for(int n0, int n1, int cnt, int tid, const F &f)
{
	while (n0 < n1) {
		const bool wide = n1 - n0 > 16;
		const int lanes = wide ? 64 : 16, per = wide ? 4 : 16;
		const int n = n0 + (tid & (lanes - 1));
		if (n < n1)
			for (int k = wide ? tid >> 6 : tid >> 4; k < cnt; k += per)
				f(n, k);
		n0 += lanes;
	}
}

// xs(r, col(c)) = fetch(r, c) for the S x S region (64 < S <= 80), neighbouring lanes on neighbouring c: a lane issues the
// loads of four rows (in the strip of the last S - 64 columns: of five) before it stores the first, so they are in flight
// together.  fetch gives 0 for a cell outside the frame.
template <class T, class Fetch, class Col>
static __device__ __forceinline__ void lift_stage(T *xs, int S, int tid, const Fetch &fetch, const Col &col)
{
	static_assert(kSmax <= 80, "the strip below holds 16 columns and five rows a lane");
	const int c = tid & 63, pc = col(c);
	for (int r0 = tid >> 6; r0 < S; r0 += 16) {
		T v[4];
#pragma unroll
		for (int u = 0; u < 4; u++)
			v[u] = r0 + 4 * u < S ? fetch(r0 + 4 * u, c) : T(0);
#pragma unroll
		for (int u = 0; u < 4; u++)
			if (r0 + 4 * u < S)
				xs[(r0 + 4 * u) * kPt + pc] = v[u];
	}
	const int c2 = 64 + (tid & 15), r2 = tid >> 4;
	if (c2 < S) {
		const int pc2 = col(c2);
		T v[5];
#pragma unroll
		for (int u = 0; u < 5; u++)
			v[u] = r2 + 16 * u < S ? fetch(r2 + 16 * u, c2) : T(0);
#pragma unroll
		for (int u = 0; u < 5; u++)
			if (r2 + 16 * u < S)
				xs[(r2 + 16 * u) * kPt + pc2] = v[u];
	}
}

// One pass (the scaling of the inverse, every step, the scaling of the forward; `scaled` false: the steps alone) along x
// (ROWS) or y of the LDS region xs, in place.  LDS index c along the pass holds sample g0 + c of a line of N; S cells are staged.  Lines: LDS indices
// [n0, n1) across the pass, line n being line ga0 + n of Na.
template <class T, bool INV, bool ROWS>
static __device__ __forceinline__ void lift_tile_pass(T *xs, const LiftTable &tb, bool scaled, int g0, int N, int S, int n0, int n1, int ga0, int Na,
	int tid)
{
	n0 = max(n0, -ga0);
	n1 = min(n1, Na - ga0);
	const int c_lo = max(0, -g0), c_hi = min(S, N - g0); // the staged cells inside the line
	const float f0 = INV ? tb.inv_scale[0] : tb.fwd_scale[0], f1 = INV ? tb.inv_scale[1] : tb.fwd_scale[1];
	const bool scales = std::is_same<T, float>::value && scaled && (f0 != 1.0f || f1 != 1.0f);
	auto scale = [&]() {
		lift_for(n0, n1, c_hi - c_lo, tid, [&](int n, int k) {
			const int c = c_lo + k;
			T *p = ROWS ? xs + n * kPt + c : xs + c * kPt + n;
			*p = lift_scaled(*p, ((g0 + c) & 1) ? f1 : f0);
		});
		__syncthreads();
	};
	if (n1 <= n0 || c_hi <= c_lo)
		return; // (uniform: the whole workgroup returns)
	if (INV && scales)
		scale();
	int rho = 0;
	for (int si = 0; si < tb.n_steps && N >= 2; si++) {
		const LiftStep &st = tb.steps[INV ? tb.n_steps - 1 - si : si];
		rho += st.reach;
		// the span of samples this step leaves correct
		const int a = g0 <= 0 ? 0 : g0 + rho, b = g0 + S >= N ? N : g0 + S - rho;
		const int first = a + ((a ^ st.parity) & 1);
		const int cnt = b > first ? (b - first + 1) >> 1 : 0;
		auto lift = [&](auto reflect) {
			lift_for(n0, n1, cnt, tid, [&](int n, int k) {
				const int g = first + 2 * k;
				if (ROWS) {
					T *xr = xs + n * kPt;
					xr[g - g0] = lift_eval<T, INV, decltype(reflect)::value>(st, g, N, [&](int i) { return xr[i - g0]; });
				} else {
					T *xc = xs + n;
					xc[(g - g0) * kPt] = lift_eval<T, INV, decltype(reflect)::value>(st, g, N, [&](int i) { return xc[(i - g0) * kPt]; });
				}
			});
		};
		// a span whose every tap lies inside the line (a tile away from both ends) reflects nothing
		if (a - st.reach >= 0 && b - 1 + st.reach < N)
			lift(std::false_type{});
		else
			lift(std::true_type{});
		__syncthreads();
	}
	if (!INV && scales)
		scale();
}

template <class T, bool INV>
__global__ __launch_bounds__(256) void k_lift_tile(const LiftTable tb, const LiftLevelArgs a)
{
	__shared__ T xs[kSmax * kPt];
	const int tid = threadIdx.x;
	const int R = tb.reach, S = kT + 2 * R;
	const int W = a.W, H = a.H;
	const int x0 = blockIdx.x * kT, y0 = blockIdx.y * kT;
	const long b = blockIdx.z;
	const int gx0 = x0 - R, gy0 = y0 - R; // LDS (r, c) holds sample (gy0 + r, gx0 + c)
	const T *in = (const T *)a.in + b * a.bi_in;
	T *det = (T *)a.det + b * a.bi_det;
	T *out = (T *)a.out + b * a.bi_out;

	if constexpr (!INV) {
		// 1. the tile with its halo (zeros outside the frame; the steps never read those)
		lift_stage(xs, S, tid, [&](int r, int c) {
			const int gy = gy0 + r, gx = gx0 + c;
			return gy >= 0 && gy < H && gx >= 0 && gx < W ? in[(long)gy * a.pin + gx] : T(0); }, [](int c) { return c; });
		__syncthreads();
		// 2. rows: every line of the region; 3. columns: the tile's own
		lift_tile_pass<T, false, true>(xs, tb, true, gx0, W, S, 0, S, gy0, H, tid);
		// (the column pass scales on the way out: its steps only)
		lift_tile_pass<T, false, false>(xs, tb, false, gy0, H, S, R, R + kT, gx0, W, tid);
		// 4. the four subbands, each a run of rows: lanes along x
		for (int q = 0; q < 4; q++) {
			const int py = q >> 1, px = q & 1;
			const float f = tb.fwd_scale[py];
			for (int e = tid; e < (kT / 2) * (kT / 2); e += 256) {
				const int gx = x0 + 2 * (e % (kT / 2)) + px, gy = y0 + 2 * (e / (kT / 2)) + py;
				if (gx >= W || gy >= H)
					continue;
				const T v = lift_scaled(xs[(gy - gy0) * kPt + gx - gx0], f);
				const int ox = lift_pos(gx, W), oy = lift_pos(gy, H);
				if (q == 0)
					out[(long)oy * a.pout + ox] = v;
				else
					det[(long)oy * a.pd + ox] = v;
			}
		}
	} else {
		// 1. the four subbands under the region, each from its Mallat place: the lanes of a half row read neighbours
		const int half = S >> 1;
		auto col = [&](int cc) { return cc < half ? 2 * cc : 2 * (cc - half) + 1; };
		lift_stage(xs, S, tid, [&](int r, int cc) {
			const int gy = gy0 + r, gx = gx0 + col(cc);
			if (gy < 0 || gy >= H || gx < 0 || gx >= W)
				return T(0);
			const int ox = lift_pos(gx, W), oy = lift_pos(gy, H);
			return ((gx | gy) & 1) ? det[(long)oy * a.pd + ox] : in[(long)oy * a.pin + ox]; }, col);
		__syncthreads();
		// 2. the first pass over every line of the region, the second over the tile's own
		if (tb.inv_cols_first) {
			lift_tile_pass<T, true, false>(xs, tb, true, gy0, H, S, 0, S, gx0, W, tid);
			lift_tile_pass<T, true, true>(xs, tb, true, gx0, W, S, R, R + kT, gy0, H, tid);
		} else {
			lift_tile_pass<T, true, true>(xs, tb, true, gx0, W, S, 0, S, gy0, H, tid);
			lift_tile_pass<T, true, false>(xs, tb, true, gy0, H, S, R, R + kT, gx0, W, tid);
		}
		// 3. the tile
		for (int e = tid; e < kT * kT; e += 256) {
			const int gx = x0 + e % kT, gy = y0 + e / kT;
			if (gx < W && gy < H)
				out[(long)gy * a.pout + gx] = xs[(gy - gy0) * kPt + gx - gx0];
		}
	}
}

// ---- the step-by-step route ------------------------------------------------------------------------------------------

static inline dim3 lift_grid(long threads)
{
	const long b = (threads + 255) / 256;
	return dim3((unsigned)(b < 65536 ? (b > 0 ? b : 1) : 65536));
}

// W x H words of `batch` frames, src -> dst
__global__ __launch_bounds__(256) void k_lift_copy(const unsigned *__restrict__ src, long ps, long bs, unsigned *__restrict__ dst, long pd,
	long bd, int W, int H, int batch)
{
	const long total = (long)W * H * batch;
	for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
		const int x = (int)(t % W), y = (int)(t / W % H);
		const long b = t / ((long)W * H);
		dst[b * bd + (long)y * pd + x] = src[b * bs + (long)y * ps + x];
	}
}

// one step along x (rows) or y of x[batch][H][W], in place: one thread per sample of the step's parity
template <class T, bool INV>
__global__ __launch_bounds__(256) void k_lift_step(T *__restrict__ x, int W, int H, int batch, const LiftStep st, int rows)
{
	const int N = rows ? W : H, nl = rows ? H : W;
	const int cnt = st.parity ? N >> 1 : (N + 1) >> 1;
	const long total = (long)cnt * nl * batch;
	for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
		const long b = t / ((long)cnt * nl);
		const long u = t % ((long)cnt * nl);
		// lanes along x: neighbouring targets of a row, neighbouring columns
		const int k = rows ? (int)(u % cnt) : (int)(u / nl), line = rows ? (int)(u / cnt) : (int)(u % nl);
		const int g = 2 * k + st.parity;
		T *base = x + b * W * H + (rows ? (long)line * W : (long)line);
		const long es = rows ? 1 : W;
		base[g * es] = lift_eval<T, INV>(st, g, N, [&](int i) { return base[i * es]; });
	}
}

__global__ __launch_bounds__(256) void k_lift_scale(float *__restrict__ x, int W, int H, int batch, int along_x, float f0, float f1)
{
	const long total = (long)W * H * batch;
	for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
		const int gx = (int)(t % W), gy = (int)(t / W % H);
		x[t] = lift_scaled(x[t], ((along_x ? gx : gy) & 1) ? f1 : f0);
	}
}

// threads enumerate the DESTINATION of the place (Mallat order) and the SOURCE of the gather alike: lanes along a band's row
template <class T>
__global__ __launch_bounds__(256) void k_lift_place(const T *__restrict__ x, T *__restrict__ dst, long pd, long bd, int W, int H, int batch,
	float f0, float f1)
{
	const long total = (long)W * H * batch;
	const int Wd = (W + 1) >> 1, Hd = (H + 1) >> 1;
	for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
		const int ox = (int)(t % W), oy = (int)(t / W % H);
		const long b = t / ((long)W * H);
		const int gx = ox < Wd ? 2 * ox : 2 * (ox - Wd) + 1, gy = oy < Hd ? 2 * oy : 2 * (oy - Hd) + 1;
		dst[b * bd + (long)oy * pd + ox] = lift_scaled(x[b * W * H + (long)gy * W + gx], (gy & 1) ? f1 : f0);
	}
}

template <class T>
__global__ __launch_bounds__(256) void k_lift_gather(const T *__restrict__ ll, long pll, long bll, const T *__restrict__ det, long pd, long bd,
	T *__restrict__ x, int W, int H, int batch, int along_x, float f0, float f1)
{
	const long total = (long)W * H * batch;
	const int Wd = (W + 1) >> 1, Hd = (H + 1) >> 1;
	for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
		const int ox = (int)(t % W), oy = (int)(t / W % H);
		const long b = t / ((long)W * H);
		const int gx = ox < Wd ? 2 * ox : 2 * (ox - Wd) + 1, gy = oy < Hd ? 2 * oy : 2 * (oy - Hd) + 1;
		const T v = (ox < Wd && oy < Hd) ? ll[b * bll + (long)oy * pll + ox] : det[b * bd + (long)oy * pd + ox];
		x[b * W * H + (long)gy * W + gx] = lift_scaled(v, ((along_x ? gx : gy) & 1) ? f1 : f0);
	}
}

// ---- a batch of lines (dwt_hip_lifting1d_batch) -----------------------------------------------------------

// `mode` 0: W words of H lines, src -> dst as they are.  1: the lines of the source in Mallat order (L from ll, H from det)
// -> sample order, 2: sample order -> Mallat order; both scaled by the parity of the sample.  Element i of line y at
// y*ls + i*es WORDS on either side; threads enumerate the Mallat side.
template <class T>
__global__ __launch_bounds__(256) void k_lift_line_move(const T *__restrict__ ll, const T *__restrict__ det, long sls, long ses, T *__restrict__ dst,
	long dls, long des, int W, int H, int mode, float f0, float f1)
{
	const long total = (long)W * H;
	const int Wd = (W + 1) >> 1;
	for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
		const int ox = (int)(t % W);
		const long y = t / W;
		const int gx = ox < Wd ? 2 * ox : 2 * (ox - Wd) + 1;
		if (mode == 0)
			dst[y * dls + ox * des] = ll[y * sls + ox * ses];
		else if (mode == 1)
			dst[y * dls + gx * des] = lift_scaled((ox < Wd ? ll : det)[y * sls + ox * ses], (gx & 1) ? f1 : f0);
		else
			dst[y * dls + ox * des] = lift_scaled(ll[y * sls + gx * ses], (gx & 1) ? f1 : f0);
	}
}

static __host__ __device__ __forceinline__ int lift_r4(int n) { return (n + 3) & ~3; }
static __host__ __device__ __forceinline__ int lift_len(int N, int j) { return (N + (1 << j) - 1) >> j; }
// words of LDS one line takes, each part rounded up to 16 B: forward the line and the next level's input, inverse the line
// and the outputs of two consecutive levels
static __host__ __device__ __forceinline__ int lift_line_words(bool inverse, int N)
{
	return lift_r4(N) + lift_r4(lift_len(N, 1)) + (inverse ? lift_r4(lift_len(N, 2)) : 0);
}

struct LiftLinesArgs {
	const char *src;
	char *dst;
	long line_stride, elem_stride; // bytes
	int n_lines, N, levels;
	int tpl; // threads per line: 64, 128 or 256
	int vec; // dense lines whose every address is a multiple of 16 bytes
};

// Every step of one level of one line, in place.  The line of n samples lies as two parity arrays, E its even samples and
// O its odd ones, so the lanes of a step walk both with unit stride (sample 2k + p of an interleaved line would put them on
// every second bank): sample i is ((i & 1) ? O : E)[i >> 1].  A step writes one array and reads the other: one barrier a step.
template <class T, bool INV>
static __device__ __forceinline__ void lift_line_steps(const LiftTable &tb, T *E, T *O, int n, int t, int tpl, bool active)
{
	auto at = [&](int i) { return ((i & 1) ? O : E)[i >> 1]; };
	for (int si = 0; si < tb.n_steps && n >= 2; si++) {
		const LiftStep &st = tb.steps[INV ? tb.n_steps - 1 - si : si];
		T *const own = st.parity ? O : E;
		const int cnt = st.parity ? n >> 1 : (n + 1) >> 1;
		if (active)
			for (int k = t; k < cnt; k += tpl) {
				const int g = 2 * k + st.parity;
				// a sample whose every tap lies inside the line reflects nothing
				own[k] = g >= st.reach && g + st.reach < n ? lift_eval<T, INV, false>(st, g, n, at) : lift_eval<T, INV, true>(st, g, n, at);
			}
		__syncthreads();
	}
}

// Every level of `n_lines` lines of N <= N1D_MAX samples in ONE launch, any scheme of any reach: a line lies in LDS whole,
// so there is no halo.  `tpl` threads work on a line, 256 / tpl lines share the workgroup; all lines have the same length and
// depth, so every thread meets the same barriers.
// Forward: the line is split by parity as it arrives -- even samples at [0, ceil(n/2)), odd ones behind them, which are
// the level's Mallat places.  Per level the steps run in place; H, scaled, goes to its Mallat offset in global memory; L,
// scaled, is split by parity into the other buffer, the next level's input; the last level's L goes to global memory.
// Inverse: the whole line is loaded (line_to_lds) and scaled once, L_J by inv_scale[0], every H band by inv_scale[1].  A
// level's E is its L part -- the previous level's output, the line's prefix at the coarsest level --, its O is its H band
// where it was loaded; after the steps the two are interleaved, scaled by inv_scale[0] as the next level's L, into the
// other buffer (the finest level: into global memory, unscaled).
template <class T, bool INV>
__global__ __launch_bounds__(256) void k_lift_lines(const LiftTable tb, const LiftLinesArgs a)
{
	extern __shared__ float lift_lds[];
	constexpr bool kFloat = std::is_same<T, float>::value;
	using V2 = typename std::conditional<kFloat, float2, int2>::type;
	using V4 = typename std::conditional<kFloat, float4, int4>::type;
	const int tpl = a.tpl, N = a.N;
	const int sub = threadIdx.x / tpl, t = threadIdx.x % tpl;
	const long line = (long)blockIdx.x * (blockDim.x / tpl) + sub;
	const bool active = line < a.n_lines;
	T *const A = (T *)lift_lds + (long)sub * lift_line_words(INV, N);
	T *const B = A + lift_r4(N);
	const char *s = a.src + line * a.line_stride;
	char *d = a.dst + line * a.line_stride;
	const long es = a.elem_stride;
	auto ld = [&](int i) { return *(const T *)(s + i * es); };
	auto st = [&](int i, T v) { *(T *)(d + i * es) = v; };

	if constexpr (!INV) {
		if (active) {
			const int nl = (N + 1) >> 1;
			const int n4 = a.vec ? N >> 2 : 0;
			for (int i = t; i < n4; i += tpl) {
				const V4 v = *(const V4 *)(s + 16l * i);
				A[2 * i] = v.x, A[2 * i + 1] = v.z, A[nl + 2 * i] = v.y, A[nl + 2 * i + 1] = v.w;
			}
			for (int i = 4 * n4 + t; i < N; i += tpl)
				A[lift_pos(i, N)] = ld(i);
		}
		__syncthreads();
		T *cur = A, *nxt = B;
		int n = N;
		for (int lev = 0; lev < a.levels; lev++) {
			const int nl = (n + 1) >> 1, nh = n >> 1;
			const bool last = lev == a.levels - 1;
			T *const E = cur, *const O = cur + nl;
			lift_line_steps<T, false>(tb, E, O, n, t, tpl, active);
			if (active) {
				for (int k = t; k < nh; k += tpl)
					st(nl + k, lift_scaled(O[k], tb.fwd_scale[1])); // H: final, to its Mallat offset
				for (int k = t; k < nl; k += tpl) {
					const T v = lift_scaled(E[k], tb.fwd_scale[0]);
					if (last)
						st(k, v);
					else
						nxt[lift_pos(k, nl)] = v;
				}
			}
			if (!last)
				__syncthreads();
			cur = nxt, nxt = E, n = nl;
		}
	} else {
		T *const C = B + lift_r4(lift_len(N, 1));
		if (active) {
			if constexpr (kFloat) {
				line_to_lds(A, s, N, es, t, tpl, a.vec);
			} else {
				const int n4 = a.vec ? N >> 2 : 0;
				for (int i = t; i < n4; i += tpl)
					*(V4 *)(A + 4 * i) = *(const V4 *)(s + 16l * i);
				for (int i = 4 * n4 + t; i < N; i += tpl)
					A[i] = ld(i);
			}
		}
		__syncthreads();
		if (kFloat && (tb.inv_scale[0] != 1.0f || tb.inv_scale[1] != 1.0f)) {
			const int nj = lift_len(N, a.levels);
			if (active)
				for (int i = t; i < N; i += tpl)
					A[i] = lift_scaled(A[i], tb.inv_scale[i < nj ? 0 : 1]);
			__syncthreads();
		}
		for (int lev = a.levels - 1; lev >= 0; lev--) {
			const int n = lift_len(N, lev), nl = (n + 1) >> 1, nh = n >> 1;
			T *const E = lev == a.levels - 1 ? A : ((lev + 1) & 1) ? B : C;
			T *const O = A + nl;
			T *const out = (lev & 1) ? B : C; // (lev >= 1: B holds ceil(N/2) samples, C ceil(N/4))
			lift_line_steps<T, true>(tb, E, O, n, t, tpl, active);
			if (active)
				for (int k = t; k < nl; k += tpl) {
					if (lev > 0) {
						const T e = lift_scaled(E[k], tb.inv_scale[0]);
						if (k < nh) {
							V2 v;
							v.x = e, v.y = lift_scaled(O[k], tb.inv_scale[0]);
							*(V2 *)(out + 2 * k) = v;
						} else {
							out[2 * k] = e;
						}
					} else if (a.vec && k < nh) {
						V2 v;
						v.x = E[k], v.y = O[k];
						*(V2 *)(d + 8l * k) = v;
					} else {
						st(2 * k, E[k]);
						if (k < nh)
							st(2 * k + 1, O[k]);
					}
				}
			if (lev > 0)
				__syncthreads();
		}
	}
}

} // namespace

hipError_t launch_lift_lines(bool inverse, const LiftTable &tb, const void *src, void *dst, long line_stride, long elem_stride, int n_lines,
	int N, int levels, hipStream_t s)
{
	// (levels <= 30: 1 << level stays inside int)
	if (n_lines < 1 || levels < 1 || levels > 30 || N < 1 || N > N1D_MAX || elem_stride < 4 || elem_stride % 4 || line_stride % 4)
		return hipErrorInvalidValue;
	LiftLinesArgs a;
	a.src = (const char *)src, a.dst = (char *)dst, a.line_stride = line_stride, a.elem_stride = elem_stride;
	a.n_lines = n_lines, a.N = N, a.levels = levels;
	// threads per line: one wave for short lines (four lines per workgroup), the whole workgroup for long ones
	a.tpl = N <= LIFT_LINE_WAVE ? 64 : N <= LIFT_LINE_HALF ? 128 : 256;
	a.vec = elem_stride == 4 && line_stride % 16 == 0 && (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0;
	const int lpw = 256 / a.tpl;
	const size_t lds = (size_t)lpw * lift_line_words(inverse, N) * 4;
	// (no cap on n_lines: an int's worth of lines is fewer workgroups than grid.x takes)
	const dim3 grid((unsigned)(((long)n_lines + lpw - 1) / lpw));
	if (tb.is_int) {
		if (inverse)
			k_lift_lines<int, true><<<grid, 256, lds, s>>>(tb, a);
		else
			k_lift_lines<int, false><<<grid, 256, lds, s>>>(tb, a);
	} else {
		if (inverse)
			k_lift_lines<float, true><<<grid, 256, lds, s>>>(tb, a);
		else
			k_lift_lines<float, false><<<grid, 256, lds, s>>>(tb, a);
	}
	return hipGetLastError();
}

hipError_t launch_lift_line_move(int mode, const void *ll, const void *det, long sls, long ses, void *dst, long dls, long des, int W, int H,
	bool scale, float f0, float f1, hipStream_t s)
{
	const dim3 grid = lift_grid((long)W * H);
	if (scale && mode != 0)
		k_lift_line_move<float><<<grid, 256, 0, s>>>((const float *)ll, (const float *)det, sls, ses, (float *)dst, dls, des, W, H, mode, f0, f1);
	else
		k_lift_line_move<int><<<grid, 256, 0, s>>>((const int *)ll, (const int *)det, sls, ses, (int *)dst, dls, des, W, H, mode, 1.0f, 1.0f);
	return hipGetLastError();
}

hipError_t launch_lift_tile(bool inverse, const LiftTable &tb, const LiftLevelArgs &a, hipStream_t s)
{
	if (a.W < 1 || a.H < 1 || a.batch < 1 || a.batch > 65535 || tb.reach < 0 || tb.reach > LIFT_FUSED_REACH)
		return hipErrorInvalidValue;
	const dim3 grid((a.W + kT - 1) / kT, (a.H + kT - 1) / kT, a.batch);
	if (grid.y > 65535)
		return hipErrorInvalidValue;
	if (tb.is_int) {
		if (inverse)
			k_lift_tile<int, true><<<grid, 256, 0, s>>>(tb, a);
		else
			k_lift_tile<int, false><<<grid, 256, 0, s>>>(tb, a);
	} else {
		if (inverse)
			k_lift_tile<float, true><<<grid, 256, 0, s>>>(tb, a);
		else
			k_lift_tile<float, false><<<grid, 256, 0, s>>>(tb, a);
	}
	return hipGetLastError();
}

hipError_t launch_lift_copy(const void *src, long ps, long bs, void *dst, long pd, long bd, int W, int H, int batch, hipStream_t s)
{
	k_lift_copy<<<lift_grid((long)W * H * batch), 256, 0, s>>>((const unsigned *)src, ps, bs, (unsigned *)dst, pd, bd, W, H, batch);
	return hipGetLastError();
}

hipError_t launch_lift_step(bool is_int, bool inverse, void *x, int W, int H, int batch, const LiftStep &st, bool rows, hipStream_t s)
{
	const int N = rows ? W : H;
	const dim3 grid = lift_grid((long)((N + 1) >> 1) * (rows ? H : W) * batch);
	if (is_int) {
		if (inverse)
			k_lift_step<int, true><<<grid, 256, 0, s>>>((int *)x, W, H, batch, st, rows);
		else
			k_lift_step<int, false><<<grid, 256, 0, s>>>((int *)x, W, H, batch, st, rows);
	} else {
		if (inverse)
			k_lift_step<float, true><<<grid, 256, 0, s>>>((float *)x, W, H, batch, st, rows);
		else
			k_lift_step<float, false><<<grid, 256, 0, s>>>((float *)x, W, H, batch, st, rows);
	}
	return hipGetLastError();
}

hipError_t launch_lift_scale(void *x, int W, int H, int batch, bool along_x, float f0, float f1, hipStream_t s)
{
	k_lift_scale<<<lift_grid((long)W * H * batch), 256, 0, s>>>((float *)x, W, H, batch, along_x, f0, f1);
	return hipGetLastError();
}

hipError_t launch_lift_place(const void *x, void *dst, long pd, long bd, int W, int H, int batch, bool scale, float f0, float f1, hipStream_t s)
{
	const dim3 grid = lift_grid((long)W * H * batch);
	if (scale)
		k_lift_place<float><<<grid, 256, 0, s>>>((const float *)x, (float *)dst, pd, bd, W, H, batch, f0, f1);
	else
		k_lift_place<int><<<grid, 256, 0, s>>>((const int *)x, (int *)dst, pd, bd, W, H, batch, 1.0f, 1.0f);
	return hipGetLastError();
}

hipError_t launch_lift_gather(const void *ll, long pll, long bll, const void *det, long pd, long bd, void *x, int W, int H, int batch,
	bool scale, bool along_x, float f0, float f1, hipStream_t s)
{
	const dim3 grid = lift_grid((long)W * H * batch);
	if (scale)
		k_lift_gather<float><<<grid, 256, 0, s>>>((const float *)ll, pll, bll, (const float *)det, pd, bd, (float *)x, W, H, batch, along_x, f0, f1);
	else
		k_lift_gather<int><<<grid, 256, 0, s>>>((const int *)ll, pll, bll, (const int *)det, pd, bd, (int *)x, W, H, batch, along_x, 1.0f, 1.0f);
	return hipGetLastError();
}

} // namespace dwt
