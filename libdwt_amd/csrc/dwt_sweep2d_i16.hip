// dwt_sweep2d_i16.hip -- the fused tile sweeps of the reversible int16 CDF 5/3 in JPEG 2000 order (Cdf53I16, dwt_lift.h):
// one launch per level of a dense Mallat frame or batch, every sample read once and every coefficient written once.
//
// It sits beside dwt_sweep2d_d.hip as that file sits beside the float sweeps: the tile origin, the streaming vertical pass
// and the grid are the shared pieces of dwt_sweep2d.h, and the byte layout of the float kernels is kept -- a lane owns
// 32 B of a row in the forward sweep (16 samples, a tile of 1024 columns) and 16 B in the inverse one (8 samples, 512
// columns), so loads and stores have the sizes those kernels were tuned for.  What differs:
//
//   - ORDER.  A forward level lifts the columns BEFORE the rows (2D_SD), so the streaming vertical pass runs first, on
//     the raw rows, and the horizontal lift follows on the two rows it completes.  The horizontal lift of a lane's 16
//     columns reads 2 columns to their left and 1 to their right; those halo columns are therefore lifted vertically by
//     the lane as well (19 columns of vertical work for 16 of output).  The inverse is the mirror: rows first, in
//     registers, then the streaming vertical pass -- the order of the other inverse sweeps.
//   - ARITHMETIC in 32-bit lanes.  A packed 16-bit add wraps before the shift, which is not the normative arithmetic once
//     l + r leaves 16 bits; samples are sign-extended on load and every step is truncated to 16 bits (Cdf53I16::sx), so a
//     step is evaluated exactly as C evaluates cdf53_vert_2x1_i16 on int-promoted operands.
//   - PER-SAMPLE HALO.  A row of odd width ends in the middle of a dword and the reflected halo is per sample: halo
//     columns and the columns of a lane that overhangs the row's end are fetched sample by sample through reflected
//     indices; only lanes whose columns all lie inside the row use 16-byte accesses.  Nothing is read or written outside
//     the W x H region of an image (no reliance on a buffer's bounds check).
//   - ALIGNMENT.  The driver sends images whose base or pitch is not a multiple of 4 bytes to the line passes, so a
//     lane's own 32 B / 16 B of an image row are dword-aligned.  The subbands right of the LL / LH quarter start at
//     sample ceil(W/2): where that is odd they are 2-byte aligned only, and those rows are accessed sample by sample
//     (a test on the address, uniform over the wave).
//   - No LDS ring: rows go straight to registers, the next iteration's rows being fetched while this one's are lifted.
#include "dwt_sweep2d.h"

namespace dwt {

namespace {

typedef u4 u4a __attribute__((aligned(4)));
typedef u2 u2a __attribute__((aligned(4)));

static __device__ __forceinline__ bool dword_aligned(const void *p) { return ((uintptr_t)p & 3) == 0; }

// sample i (0 = low half) of a packed pair
static __device__ __forceinline__ int half_of(unsigned w, int i) { return i ? (int)w >> 16 : (int)(short)w; }
static __device__ __forceinline__ unsigned pack_pair(int lo, int hi) { return ((unsigned)lo & 0xffffu) | ((unsigned)hi << 16); }

// reflection of column / sample index i into a line of N >= 2: one bounce for the lines long enough (i within 16 of
// the line), the general form otherwise
static __device__ __forceinline__ int refl_i16(int i, int N)
{
	return N >= 32 ? reflect_near(i, N) : reflect(i, N);
}

// the first n of 8 consecutive samples (packed in v) to p: one 16-byte store where all 8 are wanted and p is dword-aligned
template <bool NT>
static __device__ __forceinline__ void store_samples8(short *p, u4 v, int n)
{
	if (n >= 8 && dword_aligned(p)) {
		if constexpr (NT)
			__builtin_nontemporal_store((u4a)v, (u4a *)p);
		else
			*(u4a *)p = v;
		return;
	}
#pragma unroll
	for (int i = 0; i < 8; i++)
		if (i < n)
			p[i] = (short)half_of(v[i >> 1], i & 1);
}

} // namespace

// ---- forward ---------------------------------------------------------------------------
// what a lane fetches of the two rows of an iteration: its own 16 columns packed, and the columns c - 2, c - 1, c + 16
struct FwdRaw16 {
	u4 m[2][2];
	int h[2][3];
};

template <class W>
__global__ __launch_bounds__(256) void k_fwd_sweep_i16(FwdLevelArgs a, SweepGeom g)
{
	using T = typename W::T;
	using S = typename W::S;
	constexpr int K = W::K, CPT = 16, TW = 64 * CPT, NARR = CPT + 2 * K - 1;
	static_assert(K == 2, "the 5/3 steps");

	const int lane = threadIdx.x & 63;
	const SweepTile tile = sweep_tile(a, g);
	if (!tile.live)
		return;
	const int A = tile.A, B = tile.B;
	const int img = blockIdx.y;
	const int Wd = (a.W + 1) >> 1, Hd = (a.H + 1) >> 1;
	const int c = tile.tx * TW + lane * CPT;
	if (c >= a.W)
		return; // (no barriers and no cross-lane operations anywhere: a lane without columns just leaves)
	const bool full = c + CPT <= a.W;
	const int n_iter = (B - A) + K;
	const int q0 = A - K / 2;

	const S *in = (const S *)a.in + (long)img * a.in_bstride;
	S *out_ll = (S *)a.out_ll + (long)img * a.ll_bstride;
	S *out_h = (S *)a.out_h + (long)img * a.h_bstride;

	const int hcol[3] = {refl_i16(c - 2, a.W), refl_i16(c - 1, a.W), refl_i16(c + CPT, a.W)};
	const bool tall = a.H >= 64;

	auto fetch = [&](int it, FwdRaw16 &raw) {
#pragma unroll
		for (int rr = 0; rr < 2; rr++) {
			const int ri = 2 * (q0 + it) - 1 + rr;
			const int r = tall ? reflect1(ri, a.H) : reflect(ri, a.H);
			const S *grow = in + (long)r * a.in_pitch;
			if (full) {
				// (every row is read once, but for the few around a tile's upper edge)
				raw.m[rr][0] = __builtin_nontemporal_load((const u4a *)(grow + c));
				raw.m[rr][1] = __builtin_nontemporal_load((const u4a *)(grow + c + 8));
			} else {
				// the lane overhangs the row's end: its columns one by one, reflected
#pragma unroll
				for (int j = 0; j < CPT; j += 2) {
					const int s0 = grow[refl_i16(c + j, a.W)], s1 = grow[refl_i16(c + j + 1, a.W)];
					raw.m[rr][j >> 3][(j >> 1) & 3] = pack_pair(s0, s1);
				}
			}
#pragma unroll
			for (int e = 0; e < 3; e++)
				raw.h[rr][e] = grow[hcol[e]];
		}
	};

	T st[K][NARR];
#pragma unroll
	for (int s = 0; s < K; s++)
#pragma unroll
		for (int v = 0; v < NARR; v++)
			st[s][v] = 0;

	FwdRaw16 cur, nxt;
	fetch(0, cur);
	for (int it = 0; it < n_iter; it++) {
		if (it + 1 < n_iter)
			fetch(it + 1, nxt);
		// row[rr][j]: column c - 2 + j of the odd (rr = 0) / even (rr = 1) row of the iteration
		T row[2][NARR];
#pragma unroll
		for (int rr = 0; rr < 2; rr++) {
			row[rr][0] = cur.h[rr][0];
			row[rr][1] = cur.h[rr][1];
#pragma unroll
			for (int j = 0; j < CPT; j++)
				row[rr][2 + j] = half_of(cur.m[rr][j >> 3][(j >> 1) & 3], j & 1);
			row[rr][NARR - 1] = cur.h[rr][2];
		}
		// columns first: the vertical steps on all 19 columns (reflected rows: the policy has no end forms) ...
		T lo[NARR], hi[NARR];
		fwd_vertical<W, kColNone>(row, st, lo, hi);
		if (it >= K) {
			const int k = A + it - K;
			// ... then the rows: the completed pair of rows, entry 0 an even column
			lift_fwd_regs<W, NARR>(lo);
			lift_fwd_regs<W, NARR>(hi);
			u4 ll, hl, lh, hh;
#pragma unroll
			for (int i = 0; i < 4; i++) {
				ll[i] = pack_pair(lo[2 + 4 * i], lo[2 + 4 * i + 2]);
				hl[i] = pack_pair(lo[2 + 4 * i + 1], lo[2 + 4 * i + 3]);
				lh[i] = pack_pair(hi[2 + 4 * i], hi[2 + 4 * i + 2]);
				hh[i] = pack_pair(hi[2 + 4 * i + 1], hi[2 + 4 * i + 3]);
			}
			const int cl = c >> 1;
			const int nl = Wd - cl, nh = (a.W >> 1) - cl; // samples left in the L / H half from the lane's first
			S *top = out_h + (long)k * a.h_pitch, *bot = out_h + (long)(Hd + k) * a.h_pitch;
			store_samples8<false>(out_ll + (long)k * a.ll_pitch + cl, ll, nl); // the next level reads it: temporal
			store_samples8<true>(top + Wd + cl, hl, nh);
			if (k < (a.H >> 1)) {
				store_samples8<true>(bot + cl, lh, nl);
				store_samples8<true>(bot + Wd + cl, hh, nh);
			}
		}
		if (it + 1 < n_iter)
			cur = nxt;
	}
}

static int i16_tile_pairs(const SweepTuning &t, long ntx, int Hd, long samples, int batch, int big, long want)
{
	if (t.tile_pairs > 0)
		return t.tile_pairs;
	// tile heights as the float sweeps pick them for the same number of BYTES per row: small levels are one round of waves
	// and want short tiles, large ones tall tiles (the K-row warm-up re-reads the tile above)
	if (samples <= (2L << 20))
		return 2;
	if (samples <= (8L << 20))
		return 4;
	int tp = big;
	while (tp > 8 && ntx * ((Hd + tp - 1) / tp) * batch < want)
		tp >>= 1;
	return tp;
}

hipError_t launch_fwd_level_i16(Wavelet w, const FwdLevelArgs &a, const SweepTuning &t, hipStream_t s)
{
	if (w != kCdf53I16 || a.W < 2 || a.H < 2 || a.batch < 1 || a.interleaved)
		return hipErrorInvalidValue;
	constexpr int TW = 1024;
	SweepGeom g;
	const int Hd = (a.H + 1) / 2;
	g.ntx = (a.W + TW - 1) / TW;
	g.tile_pairs = i16_tile_pairs(t, g.ntx, Hd, (long)a.W * a.H * a.batch, a.batch, 64, 1024);
	g.swz = t.xcd_swizzle;
	g.wave_horiz = 0; // stacked tiles
	const int waves = sweep_waves(t);
	const dim3 grid = sweep_grid(g, (Hd + g.tile_pairs - 1) / g.tile_pairs, waves, a.batch);
	k_fwd_sweep_i16<Cdf53I16><<<grid, 64 * waves, 0, s>>>(a, g);
	return hipGetLastError();
}

// ---- inverse ---------------------------------------------------------------------------
// A lane owns 8 output columns c .. c + 7 (16 B per row, one store).  Source rows are Mallat rows: "L row p" = [LL | HL],
// "H row p" = [LH | HH]; interleaved sample i of a row is L[i / 2] for even i and H[i / 2] for odd i.  The horizontal
// inverse of the lane's columns reads the samples c - 1 .. c + 9.
struct InvRaw16 {
	u2 l[2], h[2]; // the lane's own 4 L and 4 H samples of the two rows
	int e[2][3];   // samples c - 1, c + 8, c + 9
};

template <class W>
__global__ __launch_bounds__(256) void k_inv_sweep_i16(InvLevelArgs a, SweepGeom g)
{
	using T = typename W::T;
	using S = typename W::S;
	constexpr int K = W::K, CPT = 8, TW = 64 * CPT, NARR = CPT + 2 * K - 1;
	static_assert(K == 2, "the 5/3 steps");

	const int lane = threadIdx.x & 63;
	const SweepTile tile = sweep_tile(a, g);
	if (!tile.live)
		return;
	const int A = tile.A, B = tile.B;
	const int img = blockIdx.y;
	const int Wd = (a.W + 1) >> 1, Hd = (a.H + 1) >> 1;
	const int c = tile.tx * TW + lane * CPT;
	if (c >= a.W)
		return;
	const bool full = c + CPT <= a.W;
	const int cl = c >> 1;
	const int n_iter = (B - A) + K;
	const int p0 = A - K / 2;

	const S *in_ll = (const S *)a.in_ll + (long)img * a.ll_bstride;
	const S *in_h = (const S *)a.in_h + (long)img * a.h_bstride;
	S *out = (S *)a.out + (long)img * a.out_bstride;

	const int ecol[3] = {refl_i16(c - 1, a.W), refl_i16(c + CPT, a.W), refl_i16(c + CPT + 1, a.W)};
	const bool tall = a.H >= 64;

	auto quad = [&](const S *p) {
		if (dword_aligned(p))
			return (u2)__builtin_nontemporal_load((const u2a *)p);
		return u2{pack_pair(p[0], p[1]), pack_pair(p[2], p[3])};
	};
	auto fetch = [&](int it, InvRaw16 &raw) {
		const int p = p0 + it;
#pragma unroll
		for (int rr = 0; rr < 2; rr++) {
			const int rs = tall ? reflect1(2 * p + rr, a.H) : reflect(2 * p + rr, a.H);
			const int sub = rs >> 1;
			const S *gl, *gh;
			if ((rs & 1) == 0) {
				gl = in_ll + (long)sub * a.ll_pitch;
				gh = in_h + (long)sub * a.h_pitch + Wd;
			} else {
				gl = in_h + (long)(Hd + sub) * a.h_pitch;
				gh = gl + Wd;
			}
			auto sample = [&](int i) { return (int)((i & 1) ? gh[i >> 1] : gl[i >> 1]); };
			if (full) {
				raw.l[rr] = quad(gl + cl);
				raw.h[rr] = quad(gh + cl);
			} else {
#pragma unroll
				for (int j = 0; j < 2; j++) {
					raw.l[rr][j] = pack_pair(sample(refl_i16(c + 4 * j, a.W)), sample(refl_i16(c + 4 * j + 2, a.W)));
					raw.h[rr][j] = pack_pair(sample(refl_i16(c + 4 * j + 1, a.W)), sample(refl_i16(c + 4 * j + 3, a.W)));
				}
			}
#pragma unroll
			for (int e = 0; e < 3; e++)
				raw.e[rr][e] = sample(ecol[e]);
		}
	};

	T st[K][1][CPT];
#pragma unroll
	for (int s = 0; s < K; s++)
#pragma unroll
		for (int v = 0; v < CPT; v++)
			st[s][0][v] = 0;

	InvRaw16 cur, nxt;
	fetch(0, cur);
	for (int it = 0; it < n_iter; it++) {
		if (it + 1 < n_iter)
			fetch(it + 1, nxt);
		const int p = p0 + it;
		// rows first: x[j] = sample c - 1 + j of the row (x[0] odd), the K steps, the lane's columns at x[1 .. 8]
		T val[2][CPT];
#pragma unroll
		for (int rr = 0; rr < 2; rr++) {
			T x[NARR];
			x[0] = cur.e[rr][0];
#pragma unroll
			for (int v = 0; v < CPT; v++)
				x[1 + v] = (v & 1) ? half_of(cur.h[rr][v >> 2], (v >> 1) & 1) : half_of(cur.l[rr][v >> 2], (v >> 1) & 1);
			x[CPT + 1] = cur.e[rr][1];
			x[CPT + 2] = cur.e[rr][2];
			lift_inv_regs<W, NARR>(x);
#pragma unroll
			for (int v = 0; v < CPT; v++)
				val[rr][v] = x[1 + v];
		}
		// then the columns: the rows 2p - 1 and 2p are final
		T odd_row[CPT], even_row[CPT];
		inv_vertical<W, kColNone>(val[0], val[1], st, 0, odd_row, even_row);
		const int pe = p, po = p - 1;
		const bool ve = pe >= A && pe < B;
		const bool vo = po >= A && po < B && (2 * po + 1 < a.H);
		const int n = a.W - c;
		if (vo) {
			const u4 v = {pack_pair(odd_row[0], odd_row[1]), pack_pair(odd_row[2], odd_row[3]), pack_pair(odd_row[4], odd_row[5]), pack_pair(odd_row[6], odd_row[7])};
			S *d = out + (long)(2 * po + 1) * a.out_pitch + c;
			if (a.temporal_out)
				store_samples8<false>(d, v, n);
			else
				store_samples8<true>(d, v, n);
		}
		if (ve) {
			const u4 v = {pack_pair(even_row[0], even_row[1]), pack_pair(even_row[2], even_row[3]), pack_pair(even_row[4], even_row[5]), pack_pair(even_row[6], even_row[7])};
			S *d = out + (long)(2 * pe) * a.out_pitch + c;
			if (a.temporal_out)
				store_samples8<false>(d, v, n);
			else
				store_samples8<true>(d, v, n);
		}
		if (it + 1 < n_iter)
			cur = nxt;
	}
}

hipError_t launch_inv_level_i16(Wavelet w, const InvLevelArgs &a, const SweepTuning &t, hipStream_t s)
{
	if (w != kCdf53I16 || a.W < 2 || a.H < 2 || a.batch < 1 || a.interleaved)
		return hipErrorInvalidValue;
	constexpr int TW = 512;
	SweepGeom g;
	const int Hd = (a.H + 1) / 2;
	g.ntx = (a.W + TW - 1) / TW;
	g.tile_pairs = i16_tile_pairs(t, g.ntx, Hd, (long)a.W * a.H * a.batch, a.batch, 32, 2048);
	g.swz = t.xcd_swizzle;
	g.wave_horiz = 0;
	const int waves = sweep_waves(t);
	const dim3 grid = sweep_grid(g, (Hd + g.tile_pairs - 1) / g.tile_pairs, waves, a.batch);
	k_inv_sweep_i16<Cdf53I16><<<grid, 64 * waves, 0, s>>>(a, g);
	return hipGetLastError();
}

} // namespace dwt
