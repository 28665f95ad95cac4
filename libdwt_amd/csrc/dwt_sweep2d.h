// dwt_sweep2d.h -- what the four tile sweeps share (dwt_sweep2d.hip forward, dwt_sweep2d_inv.hip inverse, dwt_sweep2d_d.hip
// both in double precision): the tile geometry handed to the kernels, the launchers' rules for columns per lane, tile
// height, waves and grid, and on the device a wave's tile and the streaming vertical pass; for the double-precision
// sweeps also the row-end test and the line-end state of a lane's window.
#pragma once
#include "dwt_device.h"
#include "dwt_il_strip.h"

namespace dwt {

struct SweepGeom {
	int tile_pairs, ntx, swz;
	int wave_horiz; // 1: the waves of a workgroup take horizontally adjacent tiles
	int first = 0;  // k_*_sweep_x: the leading workgroups of the launch that take border strips, not tiles
	int tile_blocks = 0; // k_*_sweep_r: the workgroups [0, tile_blocks) take tiles, the ones behind them copy blocks
};

static inline int pick_cpt(const SweepTuning &t, int W, bool inverse)
{
	if (t.cpt == 4 || t.cpt == 8)
		return t.cpt;
	// forward: 8 columns/lane gives one 16 B store per subband row; inverse: 4
	// columns/lane gives one contiguous 16 B store per output row.  Narrow levels
	// take the narrower tile so that more waves share the work.
	if (inverse)
		return 4;
	// (below 2048 columns 8/lane leaves fewer than 4 tiles per row: a workgroup of four
	// side-by-side waves would be half idle; measured 4.15 vs 4.85 TB/s on 1024 x 1024^2)
	return W >= 2048 ? 8 : 4;
}

static inline int pick_tile_pairs(const SweepTuning &t, int W, int H, int cpt, int batch, bool inverse = false, bool interleaved = false)
{
	if (t.tile_pairs > 0)
		return t.tile_pairs;
	// Measured on MI355X (scripts/sweep_levels.sh): big levels are bandwidth bound and
	// want tall tiles (the K-row warm-up re-reads the tile above: 6 % at 64 pairs);
	// levels of a few million samples are latency bound -- a wave's sweep is a serial
	// chain -- and want the shortest tiles so that all CUs work at once.
	const int Hd = (H + 1) / 2;
	// (round 2, single-image sweep of 1024^2 / 512^2 / 256^2: 2 pairs 8.7 / 8.3 / 8.0 us against
	// 10.4 / 10.0 / 9.5 us with 4 pairs -- a launch this small is one round of waves whatever the
	// tile height, and its duration is the length of one wave's serial chain)
	// (the inverse alike: 10.7 against 12.7 us for the 1024^2 and 512^2 levels of a single image)
	if ((long)W * H * batch <= (1L << 20))
		return 2;
	if ((long)W * H * batch <= (4L << 20))
		return 4;
	const long ntx = (W + 64 * cpt - 1) / (64 * cpt);
	// the inverse sweep (256-column tiles, twice the waves): 16 pairs.  Round 6, level 0 alone, rotating images, two
	// boxes (scripts/r06/inv_geometry.py): 16 against 32 pairs 103 / 107 us for one 8192^2 image, 754 / 767 us for 8,
	// 5974 / 6096 us for 64, 57 / 60 us at 8192 x 4096, 189 / 197 at 16384 x 8192, 74 / 84 at 7000 x 5000, 408 / 415 for
	// 16 x 4096^2; 8, 12, 20, 24 pairs and 512-column tiles of any height are slower (rounds 3-5 ranked 32 first on 8 images)
	// (the interleaved layout's inverse keeps 32: its in-place levels snapshot 9 rows per boundary between tile rows, and
	// twice the boundaries cost the in-place entry 13 us of 271)
	int tp = inverse ? (interleaved ? 32 : t.inv_pairs >= 2 ? t.inv_pairs : 16) : 64;
	const long want = inverse ? 2048 : 1024; // inverse tiles are half as wide
	while (tp > 8 && ntx * ((Hd + tp - 1) / tp) * batch < want)
		tp >>= 1;
	return tp;
}

// waves per workgroup, and the grid of a level of ntx x nty tiles (g.wave_horiz decided by the caller)
static inline int sweep_waves(const SweepTuning &t)
{
	return t.waves >= 1 && t.waves <= 4 ? t.waves : 4;
}

static inline dim3 sweep_grid(const SweepGeom &g, int nty, int waves, int batch)
{
	if (g.wave_horiz)
		return dim3(((g.ntx + waves - 1) / waves) * nty, batch);
	return dim3(g.ntx * ((nty + waves - 1) / waves), batch);
}

// ---- device side ---------------------------------------------------------------------------------------------------
// The tile of this wave: column tx, row pairs [A, B) of the level's (H + 1) / 2; `live`: there is such a tile (else the
// whole wave leaves; no barriers are used anywhere).  `first`, `tile_blocks`: the launch's workgroups that take no tiles
// (tile_block_id).  wv is wave-uniform on purpose: tile geometry, row indices and row pointers then live in SGPRs.
// RUN: consecutive waves take consecutive tiles across the rows' ends (the fused pair of levels: a row whose tiles are
// no multiple of the workgroup's waves leaves no wave idle); otherwise g.wave_horiz says whether a workgroup's waves sit side by side or stacked.
// (The float sweeps' test for a launch that computes a band of the level only stays with them: inside this function it
// compiles to another layout of their code.)
struct SweepTile {
	int wv, tx, ty, A, B;
	bool live;
};

template <bool RUN = false, class Args>
static __device__ __forceinline__ SweepTile sweep_tile(const Args &a, const SweepGeom &g, int first = 0, int tile_blocks = 0)
{
	SweepTile t;
	const int nwv = blockDim.x >> 6;
	t.wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
	const int bid = tile_block_id(g.swz, first, tile_blocks);
	if constexpr (RUN) {
		const int i = bid * nwv + t.wv;
		t.tx = i % g.ntx;
		t.ty = i / g.ntx;
	} else if (g.wave_horiz) {
		const int ntxb = (g.ntx + nwv - 1) / nwv;
		t.tx = (bid % ntxb) * nwv + t.wv;
		t.ty = bid / ntxb;
	} else {
		t.tx = bid % g.ntx;
		t.ty = (bid / g.ntx) * nwv + t.wv;
	}
	const int Hd = (a.H + 1) >> 1;
	t.A = t.ty * g.tile_pairs;
	t.live = false;
	if (t.A >= Hd || t.tx >= g.ntx)
		return t;
	t.B = min(t.A + g.tile_pairs, Hd);
	t.live = true;
	return t;
}

// The test "row r (any r a sweep meets) is an end of its column": r == 0 or r == H - 1 after reflection (`tall`: one
// bounce).  A closure over the level and `tall`, as the tile functions had it each: called as a plain function of
// (r, H, tall) the test compiles to another layout of the sweeps' scalar branches.  The double-precision sweeps take it
// from here; the two float sweeps keep the same lambda written out (their kernels' instruction counts move otherwise):
// a change of the rule goes to fwd_sweep_tile and inv_sweep_tile as well.
template <class Args>
static __device__ __forceinline__ auto row_end_test(const Args &a, const bool &tall)
{
	return [&](int r) {
		if (tall)
			return r == 0 || r == a.H - 1;
		const int rr = reflect(r, a.H);
		return rr == 0 || rr == a.H - 1;
	};
}

// The line ends of a row among a lane's window of NARR entries (dwt_lift.h).  Policies with explicit end forms: the
// window's end_mask -- only the tiles that hold column 0 or W - 1 have any (`h_any`, wave-uniform: the interior tiles run
// the plain lift).  J0, J1: the two entries that meet a line end when the level's width is a multiple of the lane's
// columns -- column 0 is a lane's own first column, column W - 1 a lane's own last one (entries 0 and NARR - 1 are never
// acted on); `h_simple`: no other entry of the tile does.  SelEnds: the same two entries by selection -- the lane's flags
// e0 / e1 and its coefficients kh for the steps that reach them.
// The double-precision sweeps use this struct; fwd_sweep_tile and inv_sweep_tile (dwt_sweep2d.hip, dwt_sweep2d_inv.hip) keep
// the same state and dispatch written out, because through the struct their kernels compile to other instruction counts
// (profiles/sweep_parts_isa.md): a change of the rule goes there as well.
template <class W, bool INV, int NARR, int J0, int J1>
struct RowEnds {
	using T = typename W::T;
	static constexpr unsigned kCand = (1u << J0) | (1u << J1);
	unsigned hends = 0;
	bool h_any = false, h_simple = false, e0 = false, e1 = false;
	T kh[W::K];

	// the lane's window starts at column g0 of a row of Wn; returns its end mask, for vote()
	__device__ __forceinline__ unsigned init(int g0, int Wn)
	{
		if constexpr (kIsSelEnds<W>) {
			const unsigned m = end_mask_long<NARR>(g0, Wn);
			e0 = (m >> J0) & 1;
			e1 = (m >> J1) & 1;
			sel_coefs<W, INV, J0>(kh, e0, e1);
		} else if constexpr (W::kEndForms) {
			hends = end_mask<NARR>(g0, Wn);
		}
		return hends;
	}
	// `all`: the masks of the lane's windows together (the float inverse has two); `plain`: the launch wants no end forms
	__device__ __forceinline__ void vote(unsigned all, bool plain)
	{
		if constexpr (W::kEndForms) {
			h_any = !plain && __builtin_amdgcn_ballot_w64(all != 0) != 0;
			h_simple = __builtin_amdgcn_ballot_w64((all & ~(kCand | 1u | (1u << (NARR - 1)))) != 0) == 0;
		}
	}
	// the K lifting steps of the direction over a register row (lift_fwd_regs / lift_inv_regs)
	template <unsigned CAND = ~0u>
	static __device__ __forceinline__ void steps(T (&x)[NARR], unsigned ends)
	{
		if constexpr (INV)
			lift_inv_regs<W, NARR, CAND>(x, ends);
		else
			lift_fwd_regs<W, NARR, CAND>(x, ends);
	}
	// the horizontal lift of one register row: the end forms only where the tile has a line end
	__device__ __forceinline__ void lift(T (&x)[NARR]) const
	{
		if constexpr (kIsSelEnds<W>) {
			lift_regs_sel<W, NARR, INV, J0, J1>(x, e0, e1, kh);
		} else if constexpr (!W::kEndForms) {
			steps(x, 0u);
		} else if (__builtin_expect(!h_any, 1)) {
			steps(x, 0u);
		} else if (h_simple) {
			DWT_END_PATH();
			steps<kCand>(x, hends);
		} else {
			DWT_END_PATH();
			steps(x, hends);
		}
	}
};

// ---- the streaming vertical pass -------------------------------------------------------------------------------------
// How the steps of one iteration treat the rows that are a column's ends (ve[s]: the row step s acts on is one;
// wave-uniform, almost never any): kColNone -- no row of the iteration is an end --, kColEnds -- the policy's explicit end
// forms --, kColSel -- the select form: kv[s] the step's coefficient (doubled there), the state tap gives way to -0.0.
enum ColEnds { kColNone, kColEnds, kColSel };
template <ColEnds MODE> using ColTag = std::integral_constant<ColEnds, MODE>;

template <class W, bool INV, ColEnds MODE>
static __device__ __forceinline__ typename W::T col_step(int s, const bool *ve, const typename W::T *kv,
	typename W::T c, typename W::T l, typename W::T r)
{
	if constexpr (MODE == kColSel)
		return sel_step<W, INV>(s, ve[s], kv[s], c, l, r);
	else if constexpr (INV)
		return inv_step_at<W>(s, MODE == kColEnds && ve[s], c, l, r);
	else
		return fwd_step_at<W>(s, MODE == kColEnds && ve[s], c, l, r);
}

// One iteration of the vertical lift on N columns, state st in registers.  With a and b the iteration's two rows:
// n[0] = b, n[s + 1] = step s on (s = 0: a, else st[s - 1]) with the taps st[s] and n[s]; the iteration completes n[K] and
// n[K - 1]; then st = n.
// Forward: a / b = row[0] / row[1], the odd / even row 2q-1, 2q after the horizontal pass; lo / hi: the completed rows,
// scaled.  A policy of one step predicts only: st[0], the even row 2q-2, leaves as it is.
template <class W, ColEnds MODE, int N>
static __device__ __forceinline__ void fwd_vertical(const typename W::T (&row)[2][N], typename W::T (&st)[W::K][N],
	typename W::T (&lo)[N], typename W::T (&hi)[N], const bool *ve = nullptr, const typename W::T *kv = nullptr)
{
	using T = typename W::T;
	constexpr int K = W::K;
#pragma unroll
	for (int v = 0; v < N; v++) {
		T n[K + 1];
		n[0] = row[1][v];
#pragma unroll
		for (int s = 0; s < K; s++)
			n[s + 1] = col_step<W, false, MODE>(s, ve, kv, s ? st[s - 1][v] : row[0][v], st[s][v], n[s]);
		lo[v] = W::fwd_scale(0, K == 1 ? st[0][v] : n[K]);
		hi[v] = W::fwd_scale(1, K == 1 ? n[1] : n[K - 1]);
#pragma unroll
		for (int s = 0; s < K; s++)
			st[s][v] = n[s];
	}
}

// The vertical pass of one iteration (no row of it a column end) on two adjacent columns at once, as the halves of packed
// operations: the same steps and rounding as W::fwd_step / fwd_scale (float policies with fk: c + k (l + r)).
// row[0] / row[1]: the odd / even row of the iteration; st: the streaming state; lo / hi: the scaled outputs.
// SEL: the select form of the line ends -- ve[s]: step s acts on a row that is a column's end (wave-uniform), kv[s] its
// coefficient (doubled there); the state tap gives way to -0.0 (dwt_lift.h, SelEnds).
// (K = 2 and 4; a policy of one step takes the scalar form of the sweep)
template <class W, int CPT, bool SEL = false, class T>
static __device__ __forceinline__ void vertical_pairs(const T (&row)[2][CPT], T (&st)[W::K][CPT], T (&lo)[CPT], T (&hi)[CPT],
	const bool *ve = nullptr, const T *kv = nullptr)
{
	typedef float f2 __attribute__((ext_vector_type(2)));
	constexpr int K = W::K;
	[[maybe_unused]] const f2 nz = f2{-0.0f, -0.0f};
	auto kk = [&](int s) { return SEL ? kv[s] : W::fk(s); };
	auto tap = [&](int s, f2 v) { return (SEL && ve[s]) ? nz : v; };
	const float zl = W::fwd_scale(0, 1.0f), zh = W::fwd_scale(1, 1.0f); // (the scale factors themselves)
#pragma unroll
	for (int v = 0; v < CPT; v++) {
		if (v & 2)
			continue; // (columns v and v + 2: the stores take lo[0], lo[2], lo[4], lo[6] / lo[1], lo[3], ... as consecutive registers)
		constexpr int P = 2;
		const f2 ov = f2{row[0][v], row[0][v + P]}, ev = f2{row[1][v], row[1][v + P]};
		f2 s_[K], n_[K], lo2, hi2;
#pragma unroll
		for (int i = 0; i < K; i++)
			s_[i] = f2{st[i][v], st[i][v + P]};
		n_[0] = ev;
		n_[1] = ov + kk(0) * (tap(0, s_[0]) + ev); // d1n
		if constexpr (K == 4) {
			n_[2] = s_[0] + kk(1) * (tap(1, s_[1]) + n_[1]); // s1n
			n_[3] = s_[1] + kk(2) * (tap(2, s_[2]) + n_[2]); // d2n
			const f2 s2n = s_[2] + kk(3) * (tap(3, s_[3]) + n_[3]);
			lo2 = s2n * zl;
			hi2 = n_[3] * zh;
		} else {
			const f2 s1n = s_[0] + kk(1) * (tap(1, s_[1]) + n_[1]);
			lo2 = s1n * zl;
			hi2 = n_[1] * zh;
		}
#pragma unroll
		for (int i = 0; i < K; i++) {
			st[i][v] = n_[i][0];
			st[i][v + P] = n_[i][1];
		}
		lo[v] = lo2[0];
		lo[v + P] = lo2[1];
		hi[v] = hi2[0];
		hi[v + P] = hi2[1];
	}
}

// Inverse: a / b the L / H row p as the vertical pass sees them; K == 4: st = d2[p-1], s1[p-1], d1[p-2], e[p-2] and the
// rows 2p-3 (odd) and 2p-2 (even) are final; K == 2: st = d[p-1], e[p-1], final rows 2p-1 and 2p.  A policy of one step
// keeps two rows as well, d[p-1] and the even row p-1 it is lifted from: the even row p is final as it comes.
// The state is that of all G column groups of a lane, this call's group gi (the groups side by side within a step: the
// layout the kernels' register allocation was tuned with -- grouped the other way the int 9/7 takes 14 registers more).
// (G = 1, gi = 0: the double-precision sweep, whose lane has one group.)
template <class W, ColEnds MODE, int N, int KS, int G>
static __device__ __forceinline__ void inv_vertical(const typename W::T (&a)[N], const typename W::T (&b)[N], typename W::T (&st)[KS][G][N], int gi,
	typename W::T (&odd)[N], typename W::T (&even)[N], const bool *ve = nullptr, const typename W::T *kv = nullptr)
{
	using T = typename W::T;
	constexpr int K = W::K;
#pragma unroll
	for (int v = 0; v < N; v++) {
		if constexpr (K == 1) {
			odd[v] = col_step<W, true, MODE>(0, ve, kv, st[0][gi][v], st[1][gi][v], a[v]); // o[p-1]
			even[v] = a[v];
			st[0][gi][v] = b[v];
			st[1][gi][v] = a[v];
		} else {
			T n[K + 1];
			n[0] = b[v];
#pragma unroll
			for (int s = 0; s < K; s++)
				n[s + 1] = col_step<W, true, MODE>(s, ve, kv, s ? st[s - 1][gi][v] : a[v], st[s][gi][v], n[s]);
			odd[v] = n[K];
			even[v] = n[K - 1];
#pragma unroll
			for (int s = 0; s < K; s++)
				st[s][gi][v] = n[s];
		}
	}
}

} // namespace dwt
