// dwt_window2d.hip -- windows of the inverse 2-D transform of dense Mallat frames (include/libdwt_hip.h).
//
// k_window_level: one reconstruction level over a REGION of LL(l-1), one launch for the whole batch.  A workgroup owns a
// tile of 64 x 64 samples of the level's result (tiles start at multiples of 64 of the level's own coordinates, so a
// region is cut the same way whatever window asked for it) and, like k_eaw_inv_tile (dwt_eaw.hip):
//   1. reads the four band sub-tiles under its tile ONCE, with the halo of K samples on every side that lies inside the
//      level's frame, into LDS at their INTERLEAVED places (lanes along a band's row: every load of a wave is one run);
//   2. undoes the first direction's scaling and lifting steps in place, over every line of the tile and its halo;
//   3. undoes the second direction's over the tile's own lines;
//   4. stores the tile's samples of the region, 16 bytes per lane wherever a whole aligned run of the destination
//      row belongs to the tile and element by element elsewhere (the same values either way).
// The halo is recomputed by every tile that needs it, never exchanged.  Steps, scaling, end forms and the order of the two
// directions are the policy's own (dwt_lift.h: inv_scale, inv_step_at, kInvColsFirst), evaluated on the same operands as
// k_line_pass<W, true> evaluates them on its window of 2K + 1 samples: after step s the samples within s + 1 of a cut
// edge are stale and never read again, while an edge that IS the line's end (sample 0 or N - 1) loses nothing -- there
// the step takes the end form, or both taps from the one neighbour.  A tile reads no coefficient outside
// dwt_hip_window_regions' rectangles: its halo is what the rule gives for its own samples, without the reflected part.
// A line has two samples or more at every level these entries run (the level count is bounded by the SMALLER side).
//
// k_window_copy: a rectangle of every frame of a batch, for the window of LL(J) (nothing to undo) and for the rectangle
// copy of the cross-check route.
#include "dwt_kernels.h"
#include "dwt_lift.h"

#include <algorithm>

namespace dwt {

namespace {

template <class W>
struct WinGeom {
	static constexpr int K = W::K;
	static constexpr int HK = (K + 1) & ~1;          // halo rounded up to even: LDS entry 0 is an even sample
	static constexpr int R = WINDOW_TILE + 2 * HK;   // samples of a side in LDS
	static constexpr int P = R + 1;                  // row pitch in LDS
};

// One direction of a tile: samples [ta, tb) of a line of N wanted, LDS entry c holds sample g0 + c.  [i0, i1]: the
// interleaved samples k_line_pass's windows span for them; [lo, hi]: the part of it inside the line, which is loaded.
struct WinSpan {
	int g0, ta, tb, i0, i1, lo, hi, N;
};

template <class W>
static __device__ __forceinline__ WinSpan win_span(int tile, int a, int b, int N)
{
	constexpr int K = W::K;
	WinSpan s;
	s.g0 = tile * WINDOW_TILE - WinGeom<W>::HK;
	s.ta = max(a, tile * WINDOW_TILE);
	s.tb = min(b, (tile + 1) * WINDOW_TILE);
	s.i0 = 2 * (s.ta >> 1) - K + 1;
	s.i1 = 2 * ((s.tb - 1) >> 1) + K + 1;
	s.lo = max(s.i0, 0);
	s.hi = min(s.i1, N - 1);
	s.N = N;
	return s;
}

// The work items (q, k), q < nq fastest, of a loop that 256 lanes share: lane `tid` starts at item tid and moves 256 items
// on per trip -- one division per lane and loop instead of one per item.
struct WinItems {
	int nq, dq, dk, q, k;
	__device__ __forceinline__ WinItems(int nq_, int tid) : nq(nq_ > 0 ? nq_ : 1), dq(256 % nq), dk(256 / nq), q(tid % nq), k(tid / nq) {}
	__device__ __forceinline__ void next()
	{
		q += dq, k += dk;
		if (q >= nq)
			q -= nq, k++;
	}
};

// Scaling and the K steps of one direction, in place: `n_lines` lines from line `line0` on (LDS entries along the other
// direction), elements `es` words apart, lines `ls` words apart.  Lanes run ACROSS the lines, all at one sample of theirs:
// neighbouring words for the columns, words an odd pitch apart for the rows -- no bank is hit twice either way.
template <class W>
static __device__ __forceinline__ void win_lift(typename W::T *xs, int es, int ls, int line0, int n_lines, const WinSpan &sp, int tid)
{
	using T = typename W::T;
	constexpr int K = W::K;
	T *base = xs + line0 * ls - sp.g0 * es; // sample i of line q: base[q * ls + i * es]
	if constexpr (!std::is_integral<T>::value) {
		const int n = sp.hi - sp.lo + 1;
		for (WinItems it(n_lines, tid); it.k < n; it.next()) {
			const int i = sp.lo + it.k;
			T *p = base + it.q * ls + i * es;
			*p = W::inv_scale(i & 1, *p);
		}
		__syncthreads();
	}
#pragma unroll
	for (int s = 0; s < K; s++) {
		const int par = (s + K) & 1; // the parity inverse step s acts on (a policy of one step: the odd samples)
		const int lo = sp.i0 <= 0 ? 0 : sp.i0 + s + 1, hi = sp.i1 >= sp.N - 1 ? sp.N - 1 : sp.i1 - s - 1;
		const int first = lo + ((lo ^ par) & 1);
		const int n = hi >= first ? ((hi - first) >> 1) + 1 : 0;
		for (WinItems it(n_lines, tid); it.k < n; it.next()) {
			const int i = first + 2 * it.k;
			// at a line end both taps are the one neighbour inside the line
			const int l = i == 0 ? 1 : i - 1, r = i == sp.N - 1 ? sp.N - 2 : i + 1;
			T *p = base + it.q * ls;
			p[i * es] = inv_step_at<W>(s, i == 0 || i == sp.N - 1, p[i * es], p[l * es], p[r * es]);
		}
		__syncthreads();
	}
}

// n elements from dst on, element k = get(k): lane `lane` of `lanes` takes every lanes-th 16-byte run of the row; a run
// that lies in the row whole goes out as one access, the runs at its ends element by element
template <class S, class F>
static __device__ __forceinline__ void store_run16(S *dst, int n, int run, F get)
{
	constexpr int E = 16 / (int)sizeof(S);
	const int head = (int)(((uintptr_t)dst & 15) / sizeof(S)); // elements between the aligned address below dst and dst
	const int k0 = run * E - head;
	if (k0 >= 0 && k0 + E <= n) {
		S v[E];
#pragma unroll
		for (int j = 0; j < E; j++)
			v[j] = get(k0 + j);
		uint4 q;
		__builtin_memcpy(&q, v, 16);
		*reinterpret_cast<uint4 *>(dst + k0) = q;
	} else {
		for (int j = 0; j < E; j++)
			if (k0 + j >= 0 && k0 + j < n)
				dst[k0 + j] = get(k0 + j);
	}
}
// 16-byte runs that n elements from dst on can touch
template <class S>
static __device__ __forceinline__ int runs16(int n)
{
	constexpr int E = 16 / (int)sizeof(S);
	return (n + E - 1) / E + 1;
}

template <class W>
__global__ __launch_bounds__(256) void k_window_level(WindowLevelArgs a)
{
	using T = typename W::T;
	using S = typename storage_of<W>::type;
	using G = WinGeom<W>;
	constexpr int R = G::R, P = G::P;
	__shared__ T xs[R * P];
	const int tid = threadIdx.x;
	const int tx0 = a.xa / WINDOW_TILE, ty0 = a.ya / WINDOW_TILE;
	const int ntx = (a.xb - 1) / WINDOW_TILE - tx0 + 1, nty = (a.yb - 1) / WINDOW_TILE - ty0 + 1;
	const long tiles = (long)ntx * nty;
	for (int b = blockIdx.z; b < a.batch; b += gridDim.z) {
		const S *ll = (const S *)a.ll + (long)b * a.ll_bs;
		const S *det = (const S *)a.det + (long)b * a.det_bs;
		S *out = (S *)a.out + (long)b * a.out_bs;
		for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
			const WinSpan sx = win_span<W>(tx0 + (int)(t % ntx), a.xa, a.xb, a.W);
			const WinSpan sy = win_span<W>(ty0 + (int)(t / ntx), a.ya, a.yb, a.H);
			// 1. the four sub-tiles with their halo, each at its interleaved place
			for (int q = 0; q < 4; q++) {
				const int px = q & 1, py = q >> 1;
				const int fx = sx.lo + ((sx.lo ^ px) & 1), fy = sy.lo + ((sy.lo ^ py) & 1);
				const int nx = sx.hi >= fx ? ((sx.hi - fx) >> 1) + 1 : 0, ny = sy.hi >= fy ? ((sy.hi - fy) >> 1) + 1 : 0;
				for (WinItems it(nx, tid); nx > 0 && it.k < ny; it.next()) {
					const int gx = fx + 2 * it.q, gy = fy + 2 * it.k;
					const S v = q == 0 ? ll[(long)((gy >> 1) - a.ll_y0) * a.ll_pitch + ((gx >> 1) - a.ll_x0)]
					                   : det[(long)((py ? a.Hd : 0) + (gy >> 1)) * a.det_pitch + ((px ? a.Wd : 0) + (gx >> 1))];
					xs[(gy - sy.g0) * P + (gx - sx.g0)] = (T)v;
				}
			}
			__syncthreads();
			// 2., 3. the two directions, in the policy's order: the first over the halo lines too, the second over the tile's own
			if (W::kInvColsFirst) {
				win_lift<W>(xs, P, 1, sx.lo - sx.g0, sx.hi - sx.lo + 1, sy, tid);
				win_lift<W>(xs, 1, P, sy.ta - sy.g0, sy.tb - sy.ta, sx, tid);
			} else {
				win_lift<W>(xs, 1, P, sy.lo - sy.g0, sy.hi - sy.lo + 1, sx, tid);
				win_lift<W>(xs, P, 1, sx.ta - sx.g0, sx.tb - sx.ta, sy, tid);
			}
			// 4. the tile's samples
			const int n = sx.tb - sx.ta, rows = sy.tb - sy.ta, nr = runs16<S>(n);
			for (WinItems it(nr, tid); it.k < rows; it.next()) {
				const int gy = sy.ta + it.k;
				const T *row = xs + (gy - sy.g0) * P + (sx.ta - sx.g0);
				store_run16<S>(out + (long)(gy - a.ya) * a.out_pitch + (sx.ta - a.xa), n, it.q, [&](int k) { return (S)row[k]; });
			}
			__syncthreads(); // (the next tile's loads overwrite what these stores read)
		}
	}
}

template <class S>
__global__ __launch_bounds__(256) void k_window_copy(const S *__restrict__ src, long sp, long sbs, S *__restrict__ dst, long dp, long dbs, int w, int h,
	int batch)
{
	const int nr = runs16<S>(w);
	const int run = blockIdx.x * 256 + threadIdx.x;
	if (run >= nr)
		return;
	for (int b = blockIdx.z; b < batch; b += gridDim.z)
		for (int y = blockIdx.y; y < h; y += gridDim.y) {
			const S *s = src + b * sbs + y * sp;
			store_run16<S>(dst + b * dbs + y * dp, w, run, [&](int k) { return s[k]; });
		}
}

template <class W>
static hipError_t window_level_t(const WindowLevelArgs &a, hipStream_t s)
{
	const long ntx = (a.xb - 1) / WINDOW_TILE - a.xa / WINDOW_TILE + 1, nty = (a.yb - 1) / WINDOW_TILE - a.ya / WINDOW_TILE + 1;
	const long tiles = ntx * nty;
	const dim3 grid((unsigned)std::min(tiles, 1l << 30), 1, (unsigned)std::min(a.batch, WINDOW_GRID_BATCH));
	k_window_level<W><<<grid, 256, 0, s>>>(a);
	return hipGetLastError();
}

} // namespace

hipError_t launch_window_level(Wavelet w, const WindowLevelArgs &a, hipStream_t s)
{
	if (a.batch <= 0 || a.W < 2 || a.H < 2 || a.xa < 0 || a.ya < 0 || a.xb <= a.xa || a.yb <= a.ya || a.xb > a.W || a.yb > a.H)
		return hipErrorInvalidValue;
	switch (w) {
	case kCdf97S: return window_level_t<Cdf97S>(a, s);
	case kCdf53S: return window_level_t<Cdf53S>(a, s);
	case kInterp53S: return window_level_t<Interp53S>(a, s);
	case kCdf53I: return window_level_t<Cdf53I>(a, s);
	case kCdf53I16: return window_level_t<Cdf53I16>(a, s);
	default: break;
	}
	return hipErrorInvalidValue;
}

hipError_t launch_window_copy(int es, const void *src, long src_pitch, long src_bs, void *dst, long dst_pitch, long dst_bs, int w, int h,
	int batch, hipStream_t s)
{
	if (w <= 0 || h <= 0 || batch <= 0)
		return hipSuccess;
	const dim3 grid((unsigned)(((es == 2 ? w / 8 : w / 4) + 2 + 255) / 256), (unsigned)std::min(h, 16384), (unsigned)std::min(batch, WINDOW_GRID_BATCH));
	if (es == 2)
		k_window_copy<short><<<grid, 256, 0, s>>>((const short *)src, src_pitch, src_bs, (short *)dst, dst_pitch, dst_bs, w, h, batch);
	else if (es == 4)
		k_window_copy<int><<<grid, 256, 0, s>>>((const int *)src, src_pitch, src_bs, (int *)dst, dst_pitch, dst_bs, w, h, batch);
	else
		return hipErrorInvalidValue;
	return hipGetLastError();
}

} // namespace dwt
