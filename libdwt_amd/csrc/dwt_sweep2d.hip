// dwt_sweep2d.hip -- hand-written gfx950 (CDNA4, wave64) kernels of the 2-D lifting DWT.
//
// Two families:
//
//  1. k_line_pass: a generic out-of-place 1-D pass, one thread per output pair,
//     exact reference semantics for any line length.  Used for sparse frames
//     (size_o != size_i), single-line directions and as a cross-check variant.
//     It restates dwt_cdf97_f_ex_stride_s / _i_ex_stride_s and the 5/3 siblings
//     (src/libdwt.c:10744, 11530, 10950, 11749, 10986, 11785).
//
//  2. k_fwd_sweep / k_inv_sweep: one decomposition level of the 2-D drivers
//     (src/libdwt.c:12812-12919 forward, :17074-17176 inverse, :16334-16383,
//     :18165-18215 for 5/3) fused into a single tile sweep.  Each WAVE owns a tile
//     of 64*CPT columns and marches down its rows:
//       - input rows are streamed HBM -> LDS by asynchronous LDS-DMA
//         (global_load_lds) into a wave-private ring, several rows ahead, counted
//         with s_waitcnt vmcnt(N) -- no barriers, no VGPR staging;
//       - each lane reads its columns plus the 4-sample halo from LDS and lifts
//         them horizontally in registers;
//       - the vertical lifting state (4 partial rows for 9/7, 2 for 5/3) stays in
//         registers for the whole sweep, so every input sample is read from HBM
//         once per level and every coefficient written once;
//       - the Mallat de-interleave is done in registers, each subband row leaving
//         the wave as one contiguous 16 B/lane store.
//     Image borders use whole-sample symmetric reflection applied to the SOURCE
//     address of the DMA, so the arithmetic needs no edge cases.
//
// What this sweep shares with the inverse and the double-precision ones -- a wave's tile, the streaming vertical pass,
// the launch grid -- lives in dwt_sweep2d.h; loaders, LDS reads, stores and the fused pair of levels are this file's own,
// and so are its line-end state and row-end test (the double sweeps take theirs from the header: fwd_sweep_tile says why).
//
// Arithmetic order follows the reference exactly (rows before columns, etc.) and
// this file is compiled with -ffp-contract=off, so float results are bit-identical
// to libdwt's CPU path; int results are exact.
#include "dwt_sweep2d.h"

namespace dwt {

// ---------------------------------------------------------------------------------
// 1. generic exact line pass
// ---------------------------------------------------------------------------------
template <class W, bool INV>
__global__ __launch_bounds__(256) void k_line_pass(const char *__restrict__ src, char *__restrict__ dst,
	long line_stride, long elem_stride, int n_lines, int N, int hoff, int lanes_along_lines)
{
	using T = typename W::T;
	using S = typename storage_of<W>::type; // (the int16 5/3 lifts in int what it keeps as short)
	constexpr int K = W::K;
	const int fast = blockIdx.x * blockDim.x + threadIdx.x;
	const int slow = blockIdx.y;
	const int line = lanes_along_lines ? fast : slow;
	const int k = lanes_along_lines ? slow : fast;
	const int npairs = (N + 1) >> 1;
	if (line >= n_lines || k >= npairs)
		return;
	const char *s = src + (long)line * line_stride;
	char *d = dst + (long)line * line_stride;
	auto ld = [&](int idx) { return (T) * (const S *)(s + (long)idx * elem_stride); };
	auto st = [&](int idx, T v) { *(S *)(d + (long)idx * elem_stride) = (S)v; };
	const bool il = hoff < 0; // interleaved layout on both sides: L_k at 2k, H_k at 2k+1

	if (N == 1) {
		// the float kernels scale a lone sample, the int kernel leaves it
		if (W::kScaleSingle)
			st(0, INV ? W::inv_single(ld(0)) : W::fwd_single(ld(0)));
		return;
	}
	T w[2 * K + 1];
	if (!INV) {
		// w[j] = a[2k-K+F+j]; w[0] is an even sample (F = 1 for a policy of one step, whose window is 2k .. 2k+2)
		constexpr int F = K & 1;
#pragma unroll
		for (int j = 0; j <= 2 * K; j++)
			w[j] = ld(reflect(2 * k - K + F + j, N));
		lift_fwd_regs<W, 2 * K + 1>(w, W::kEndForms ? end_mask<2 * K + 1>(2 * k - K + F, N) : 0u);
		st(il ? 2 * k : k, W::fwd_scale(0, w[K - F]));
		if (2 * k + 1 < N)
			st(il ? 2 * k + 1 : hoff + k, W::fwd_scale(1, w[K + 1 - F]));
	} else {
		// w[j] = a[2k-K+1+j] of the interleaved signal; w[0] is an odd sample (an even one for a policy of one step, whose
		// step 0 undoes the predict on odd samples)
#pragma unroll
		for (int j = 0; j <= 2 * K; j++) {
			const int i = reflect(2 * k - K + 1 + j, N);
			const T raw = il ? ld(i) : (i & 1) ? ld(hoff + (i >> 1)) : ld(i >> 1);
			w[j] = W::inv_scale(i & 1, raw);
		}
		lift_inv_regs<W, 2 * K + 1>(w, W::kEndForms ? end_mask<2 * K + 1>(2 * k - K + 1, N) : 0u);
		st(2 * k, w[K - 1]);
		if (2 * k + 1 < N)
			st(2 * k + 1, w[K]);
	}
}

template <class W>
static hipError_t line_pass_t(bool inverse, const void *src, void *dst, long line_stride, long elem_stride,
	int n_lines, int N, int hoff, bool lanes_along_lines, hipStream_t s)
{
	if (n_lines <= 0 || N <= 0)
		return hipSuccess;
	const int npairs = (N + 1) >> 1;
	const int fast = lanes_along_lines ? n_lines : npairs;
	const int slow = lanes_along_lines ? npairs : n_lines;
	const int bs = fast >= 256 ? 256 : 64;
	dim3 grid((fast + bs - 1) / bs, slow);
	if (inverse)
		k_line_pass<W, true><<<grid, bs, 0, s>>>((const char *)src, (char *)dst, line_stride, elem_stride, n_lines, N, hoff, lanes_along_lines);
	else
		k_line_pass<W, false><<<grid, bs, 0, s>>>((const char *)src, (char *)dst, line_stride, elem_stride, n_lines, N, hoff, lanes_along_lines);
	return hipGetLastError();
}

hipError_t launch_line_pass(Wavelet w, bool inverse, const void *src, void *dst, long line_stride, long elem_stride,
	int n_lines, int N, int hoff, bool lanes_along_lines, hipStream_t s)
{
	switch (w) {
	case kCdf97S: return line_pass_t<Cdf97S>(inverse, src, dst, line_stride, elem_stride, n_lines, N, hoff, lanes_along_lines, s);
	case kCdf53I: return line_pass_t<Cdf53I>(inverse, src, dst, line_stride, elem_stride, n_lines, N, hoff, lanes_along_lines, s);
	case kCdf53S: return line_pass_t<Cdf53S>(inverse, src, dst, line_stride, elem_stride, n_lines, N, hoff, lanes_along_lines, s);
	case kCdf97D: return line_pass_t<Cdf97D>(inverse, src, dst, line_stride, elem_stride, n_lines, N, hoff, lanes_along_lines, s);
	case kCdf53D: return line_pass_t<Cdf53D>(inverse, src, dst, line_stride, elem_stride, n_lines, N, hoff, lanes_along_lines, s);
	case kCdf97I: return line_pass_t<Cdf97I>(inverse, src, dst, line_stride, elem_stride, n_lines, N, hoff, lanes_along_lines, s);
	case kCdf53SNew: return line_pass_t<Cdf53SNew>(inverse, src, dst, line_stride, elem_stride, n_lines, N, hoff, lanes_along_lines, s);
	case kCdf97IIp: return line_pass_t<Cdf97IIp>(inverse, src, dst, line_stride, elem_stride, n_lines, N, hoff, lanes_along_lines, s);
	case kInterp53S: return line_pass_t<Interp53S>(inverse, src, dst, line_stride, elem_stride, n_lines, N, hoff, lanes_along_lines, s);
	case kCdf53I16: return line_pass_t<Cdf53I16>(inverse, src, dst, line_stride, elem_stride, n_lines, N, hoff, lanes_along_lines, s);
	// (binary16 storage: the driver runs Cdf97S on a binary32 copy of the level's frame, so that a level rounds once)
	case kCdf97H: break;
	// the contracted variant exists for the fused sweeps only: line passes of such a call are exact
	case kCdf97SFma: return line_pass_t<Cdf97S>(inverse, src, dst, line_stride, elem_stride, n_lines, N, hoff, lanes_along_lines, s);
	}
	return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------------
// 2. fused tile sweeps
// ---------------------------------------------------------------------------------
// ---- forward -------------------------------------------------------------------
// IL: write the result INTERLEAVED in place of the Mallat de-interleave (row 2k = L
// row, row 2k+1 = H row, columns interleaved alike) to `out_h`: the layout of the
// 3-D path (src/volume-dwt.c:677-725), where a batch is the slices of a volume.
// X (interleaved layout, phase-ordered wavelets): the tiles leave out the samples whose rounding depends on the
// reference's phase order -- rows 0..7 and the last 8 columns of the level -- for the strip workgroups of the
// same launch (dwt_il_strip.h).
// F01 (float 9/7 by selection, 8 columns per lane, Mallat): levels 0 AND 1 in this one sweep.  The tiles are the level-0
// sweep's own -- 512 columns, 512 apart, every lane stores what it computes, every store of an interior tile a whole run of
// 1 KiB (level 0) or 512 B (level 1) --, and nothing passes between waves:
//   - after the vertical pass a lane holds 4 samples of the LL row its iteration completes; level 1's horizontal lift
//     takes the 4 neighbours on either side from the adjacent lanes' registers (wavefront shifts).  Lanes 0 and 63 have
//     no such neighbour in the wave: theirs are PHANTOM columns, the LL columns c0/2 - 4 .. c0/2 - 1 and c0/2 + 256 ..
//     c0/2 + 259 of the neighbour tiles, which this wave computes again for itself, one LL sample per lane (lane & 7: 0..3
//     the left ones, 4..7 the right ones; the other lanes repeat them): a window of 9 input columns from LDS for each of
//     the iteration's two rows, the four lifting steps on the shrinking window (10 operations, both rows as packed
//     halves), the scale and the streaming vertical lift of that one column (4 words of state).  The operations and
//     their order are those of the main columns, so the value has the bits the neighbour tile computes for its own
//     column; lanes 0 and 63 take them by a quad broadcast.  The last column of the line can lie in a right phantom's window
//     (the tile before the last one when 0 < W mod 512 < 16): entries 5 and 7 of the window take the end form by
//     selection like the main columns' candidates.  A phantom column that does not exist (left of tile 0, right of the
//     last column) holds whatever LDS holds; level 1's end form (g0, g5, g7, g9: a select, not arithmetic) cuts it off;
//   - the row slot in LDS is [main 512 | input columns c0 - 12 .. c0 + 3 | c0 + 508 .. c0 + 523]: both halo blocks are 16
//     columns, 48 B of the neighbour tile's first or last 64-byte sector and 16 B of this tile's own, so that every
//     phantom window (c0 - 12 + 2p .. c0 - 4 + 2p; c0 + 508 + 2p .. c0 + 516 + 2p) is contiguous there.  They come by ONE
//     DMA instruction per row as the 4-column halo of the other sweeps does, 32 lanes active in place of 8: kDmaPerIter
//     and with it the vmcnt ring count stay what they are.  Temporal, like every halo load;
//   - every second iteration completes an LL row pair: level 1's horizontal lift of both rows, its vertical pass (a state
//     of 4 columns) and the stores of its four quarter rows.  Its ends of a column take the end form too, the bottom one
//     by dropping the NEWER tap: the rows this sweep computes beyond the last LL row mirror the level's input, not the band;
//   - every sample is written once (lanes right of the line's end are dropped by the row's buffer descriptor); the LL band
//     of level 0 is never written.  `out_ll` is level 1's LL band;
//   - vertically a tile warms level 1 up with 4 more iterations above (none at the top of the image: the end form cuts
//     the dependence) and flushes it with 3 more below.  Every second tile row can march the other way, from its lower edge
//     upward (the kernel's argument `updown`): the same iterations in the mirrored order, same bits -- see `up` below.
// W and H are multiples of 4 and at least 128 (both levels of 64 x 64 or more); the last column of either level can then
// be a lane's last own column or the one in the middle of its columns, and both are candidates of the selection.
// SELV: the vertical pass takes its select form in EVERY iteration (the shallow ring of the level sweeps, see there); the
// fused pair's shallow ring is for launches of tens of rounds and keeps the deep ring's two bodies.
template <class W, int CPT, int RING, int NT, bool IL, bool X, bool F01 = false, bool SELV = (RING == 8)>
static __device__ __forceinline__ void fwd_sweep_tile(const FwdLevelArgs &a, const SweepGeom &g, [[maybe_unused]] int updown = 0)
{
	static_assert(!F01 || (kIsSelEnds<W> && CPT == 8 && !IL && !X && W::K == 4 && !(NT & 8)), "the fused pair: float 9/7 by selection, Mallat");
	using T = typename W::T;
	constexpr int K = W::K;
	constexpr int kRing = RING;           // ring rows per wave (any even number)
	constexpr int kAhead = kRing / 2 - 1; // sweep iterations of DMA lookahead (2 rows each)
	constexpr int kLdAux = (NT & 2) ? 2 : 0;
	constexpr bool kNtStore = (NT & 1) != 0;
	// the LL band is read again by the next level: bit 2 keeps its stores temporal so it
	// can stay in L2 / Infinity Cache
	[[maybe_unused]] constexpr bool kNtStoreLL = kNtStore && !(NT & 4);
	// bit 3: take the 4-sample neighbour taps from the adjacent lanes' registers with
	// wavefront shifts (DPP) instead of re-reading them from LDS
	constexpr bool kShuffle = (NT & 8) != 0;
	constexpr int TW = 64 * CPT;
	// LDS row slot: [main TW | left halo 4 | right halo 4]; F01: [main TW | columns c0 - 12 .. c0 + 3 | c0 + TW - 4 .. c0 + TW + 11]
	constexpr int kHalo = F01 ? 16 : 4;
	constexpr int RS = TW + 2 * kHalo;
	constexpr int kHaloLanes = 2 * kHalo; // lanes of the row's one halo DMA
	constexpr int kHaloL = F01 ? 8 : 0, kHaloR = F01 ? kHalo + 4 : 4; // where lane 0's / lane 63's four neighbour columns sit in the halo
	// horizontal halo: K samples, rounded up to even so that the lane's window starts at an even column (a policy of one
	// step: columns c - 2 .. c + CPT + 1, whose entry 1 is lifted in vain)
	constexpr int HK = (K + 1) & ~1;
	constexpr int NARR = CPT + 2 * HK;
	constexpr int kDmaPerIter = 2 * (CPT / 4 + 1); // fewest DMA instructions an iteration issues
	// (float policies whose step is c + k (l + r) rounded product-then-sum: the horizontal lift takes both rows at once)
	constexpr bool kPairRows = kIsSelEnds<W> && std::is_same<T, float>::value && has_coef_ends<W>::value && !std::is_base_of<Cdf97SFma, W>::value;
	extern __shared__ __attribute__((aligned(16))) char smem[];

	const int lane = threadIdx.x & 63;
	const SweepTile tile = sweep_tile<F01>(a, g, X ? g.first : 0, g.tile_blocks);
	if (!tile.live)
		return;
	if (a.pair_hi > 0 && (tile.A < a.pair_lo || tile.A >= a.pair_hi))
		return; // this launch computes a band of the level only
	const int wv = tile.wv, tx = tile.tx, A = tile.A, B = tile.B;
	[[maybe_unused]] const int ty = tile.ty;
	const int img = blockIdx.y;
	const int Wd = (a.W + 1) >> 1, Hd = (a.H + 1) >> 1;
	const int c0 = tx * TW;
	// (F01) the tile's direction, wave-uniform: `up` tiles march from their lower edge to their upper one (`updown`: the odd or
	// the even tile rows), dir = -1.  Iteration `it` then takes the rows (2q + 1, 2q), q = q0 - it, in place of (2q - 1, 2q),
	// q = q0 + it: every step has its two neighbours exchanged inside a commutative sum, so the bits are those of the march
	// downward.  An upward iteration completes the L row q + 2 and the H row q + 1 (downward: both q - 2).
	[[maybe_unused]] int up = 0;
	if constexpr (F01)
		up = (updown && !((ty ^ updown) & 1)) ? 1 : 0;
	[[maybe_unused]] const int dir = 1 - 2 * up;
	// level 1's warm-up beyond the edge the tile starts at (none at the image's: the end form cuts the dependence).  An upward
	// tile starts at q = B + 4 (its LL row B + 2, the last one level 1 needs, takes the input rows up to 2 B + 8) and ends at
	// A - 6 like a downward one starts there; at the image's bottom it starts at q = Hd + 1 as a downward one at the top at -2
	const int warm = !F01 ? 0 : up ? (B < Hd ? K : 1) : (A > 0 ? K : 0);
	const int n_iter = (B - A) + K + warm + (F01 ? 3 : 0);
	const int q0 = (F01 && up) ? B + warm : A - K / 2 - warm;
	// (F01) the iterations whose rows a vertical neighbour reads too, [0, t_lo) and [t_hi, n_iter): see issue()
	[[maybe_unused]] int t_lo = 0, t_hi = 0;
	if constexpr (F01) {
		t_lo = (up ? B < Hd : A > 0) ? (updown ? 11 : K + warm) : 0;
		t_hi = (updown && (up ? A > 0 : B < Hd)) ? n_iter - 11 : n_iter;
	}
	// (F01) the row step s of iteration `it` acts on (the iteration's own two rows: s = 0 and s = -1); the other sweeps keep
	// 2 (q0 + it) - 1 - s written out where they need it, as the parent has it
	[[maybe_unused]] auto row_of_step = [&](int it, int s) { return 2 * (q0 + dir * it) - dir * (1 + s); };

	const T *in = (const T *)a.in + (long)img * a.in_bstride;
	T *out_ll = (T *)a.out_ll + (long)img * a.ll_bstride;
	T *out_h = (T *)a.out_h + (long)img * a.h_bstride;

	char *ring = smem + (size_t)wv * kRing * RS * 4;
	const unsigned ring_off = lds_offset(ring);

	// Rows are addressed as BUFFERS (a descriptor per row in scalar registers, per-lane byte
	// offsets): the hardware checks every dword against the row's length, zero-fills loads and
	// drops stores beyond it, and 16-byte accesses need only 4-byte alignment (probed:
	// scripts/archive/probes/buf_probe.hip).  So every tile -- overhanging the image or not, rows aligned
	// or not -- takes the same 16-byte path; the up to four reflected columns right of the edge
	// that a valid output can reach come by one 4-byte DMA per row.
	const int n_edge = min(4, c0 + TW - a.W); // columns of this tile's main block right of the edge (<= 0: none)
	// (SelEnds: levels of 64 x 64 and more -- no index is reflected twice, no integer division in the wave's instruction stream)
	const int edge_col = kIsSelEnds<W> ? a.W - 2 - min(lane, 3) : reflect(a.W + min(lane, 3), a.W);
	const int halo_i = F01 ? (lane < 16 ? c0 - 12 + lane : c0 + TW - 4 + (lane & 15)) : lane < 4 ? c0 - 4 + lane : c0 + TW + (lane & 3);
	const int halo_col = kIsSelEnds<W> ? reflect_near(halo_i, a.W) : reflect(halo_i, a.W);

	int islot = 0, rslot = 0; // ring slots of the next rows to fill / to consume
	const bool tall = kIsSelEnds<W> || a.H >= 64; // then a row index leaves [0,H) by less than H: one bounce
	// In place (interleaved layout, a.sh): this tile's own rows and columns come from the image -- its stores trail its
	// loads --, everything else from the snapshot: a neighbour's row as a whole from the row shell, a neighbour's
	// column of an own row from the column shell (offset in that shell's row, or -1: an own column)
	[[maybe_unused]] const bool shl = IL && a.sh.rows != nullptr;
	[[maybe_unused]] int halo_sh = -1;
	if (IL && shl)
		halo_sh = (halo_col >= c0 - 4 && halo_col < c0) ? 8 * (tx - 1) + (halo_col - (c0 - 4))
			: (halo_col >= c0 + TW && halo_col < c0 + TW + 4) ? 8 * tx + 4 + (halo_col - (c0 + TW)) : -1;
	auto issue = [&](int it) {
#pragma unroll
		for (int rr = 0; rr < 2; rr++) {
			int ri = 2 * (q0 + it) - 1 + rr;
			if constexpr (F01)
				ri = row_of_step(it, -rr);
			const int r = tall ? reflect1(ri, a.H) : reflect(ri, a.H);
			char *lrow = ring + (size_t)(islot + rr) * RS * 4;
			const T *grow = in + (long)r * a.in_pitch;
			[[maybe_unused]] const T *hsrc = grow + halo_col; // lanes 0..7 (F01: 0..31): the halo column
			// (in place) an own row read from the image: its last 8 columns -- the border strip waves of the launch may
			// have written theirs already -- come from the snapshot `rgt + column`
			[[maybe_unused]] const T *rgt = nullptr;
			if (IL && shl) {
				if (r < 2 * A)
					grow = (const T *)a.sh.rows + (long)(9 * (ty - 1) + r - (2 * A - 5)) * a.sh.rows_pitch, hsrc = grow + halo_col;
				else if (r >= 2 * B)
					grow = (const T *)a.sh.rows + (long)(9 * ty + r - (2 * B - 5)) * a.sh.rows_pitch, hsrc = grow + halo_col;
				else if (r < kIlKeepTop) // the strips' rows: the snapshot of rows 0..13
					grow = (const T *)a.sh.top + (long)r * a.sh.top_pitch, hsrc = grow + halo_col;
				else {
					rgt = (const T *)a.sh.right + (long)r * a.sh.right_pitch - a.sh.right_x0;
					if (halo_sh >= 0)
						hsrc = (const T *)a.sh.cols + (long)r * a.sh.cols_pitch + halo_sh;
					else if (halo_col >= a.W - kIlKeepRight)
						hsrc = rgt + halo_col;
				}
			}
			[[maybe_unused]] const T *esrc = (IL && rgt) ? rgt + edge_col : grow + edge_col; // lanes < n_edge: a reflected column
			const bool fix_right = IL && rgt && c0 + TW > a.W - kIlKeepRight; // this tile holds the last 8 columns
			const row_rsrc_t rs = row_rsrc(grow, (unsigned)a.W * 4);
			// The 8 rows around a tile's upper edge are read twice: by this tile now, in its warm-up, and by the
			// tile above at the end of its march.  The first read is TEMPORAL whatever the policy, so that the
			// lines can wait in the Infinity Cache for the second one (every other row is read once).  Round 4,
			// 32 x 8192^2, one placement: level 0 6108 -> 6240 GB/s; with the halo columns temporal too 6285.
			// (F01, `updown`) a tile and its vertical neighbour march towards their common edge or away from it together and
			// read the 22 rows around it within some 11 iterations of each other: both reads of those rows, at either end of the
			// tile, are temporal and the second one hits in L2 (profiles/fuse01_updown_summary.md: non-temporal loses 5 %).
			// The fused pair takes its rows in a statement of its own (no shells, no kept columns), so that the other sweeps keep
			// the parent's statement word for word: any other form of its test compiles to other register counts in the
			// kernels of the interleaved layout.
			if constexpr (F01) {
				auto row_dma = [&](auto aux) {
#pragma unroll
					for (int i = 0; i < CPT / 4; i++)
						dma16_row<decltype(aux)::value>(rs, (unsigned)(c0 + i * 256 + lane * 4) * 4, lrow + i * 1024);
					if (lane < n_edge)
						dma4<decltype(aux)::value>(esrc, lrow + (a.W - c0) * 4);
					if (lane < kHaloLanes)
						dma4<0>(grow + halo_col, lrow + TW * 4);
				};
				if (kLdAux != 0 && (it < t_lo || it >= t_hi))
					row_dma(std::integral_constant<int, 0>{});
				else
					row_dma(std::integral_constant<int, kLdAux>{});
			} else
			if (kLdAux != 0 && it < K + warm && A > 0) {
#pragma unroll
				for (int i = 0; i < CPT / 4; i++)
					dma16_row<0>(rs, (unsigned)(c0 + i * 256 + lane * 4) * 4, lrow + i * 1024);
				if (fix_right && lane < kIlKeepRight) // (lands after the row's own DMA: loads return in order)
					dma4<0>(rgt + (a.W - kIlKeepRight + lane), lrow + (a.W - kIlKeepRight - c0) * 4);
				if (lane < n_edge)
					dma4<0>(esrc, lrow + (a.W - c0) * 4);
				if (lane < kHaloLanes)
					dma4<0>(IL ? hsrc : grow + halo_col, lrow + TW * 4);
			} else {
#pragma unroll
				for (int i = 0; i < CPT / 4; i++)
					dma16_row<kLdAux>(rs, (unsigned)(c0 + i * 256 + lane * 4) * 4, lrow + i * 1024);
				if (fix_right && lane < kIlKeepRight)
					dma4<0>(rgt + (a.W - kIlKeepRight + lane), lrow + (a.W - kIlKeepRight - c0) * 4);
				if (lane < n_edge)
					dma4<kLdAux>(esrc, lrow + (a.W - c0) * 4);
				// (the halo columns are the x-neighbour tiles' own lines, read by them at about the same time: temporal)
				if (lane < kHaloLanes)
					dma4<0>(IL ? hsrc : grow + halo_col, lrow + TW * 4);
			}
		}
		islot = islot + 2 >= kRing ? 0 : islot + 2;
	};

	T st[K][CPT];
#pragma unroll
	for (int s = 0; s < K; s++)
#pragma unroll
		for (int v = 0; v < CPT; v++)
			st[s][v] = 0;

	// (the line-end state and its dispatch below are RowEnds of dwt_sweep2d.h written out: through the struct most of this
	// file's kernels compile to other instruction counts, and the headline's kernels stay as they were measured)
	// explicit line-end forms: which of the lane's columns c - K .. c + CPT + K - 1 are a row's ends -- only the tiles
	// that hold column 0 or W - 1 have any (`h_any`, wave-uniform: the interior tiles run the plain lift) --; the rows that
	// are a column's ends are found per iteration (wave-uniform as well)
	[[maybe_unused]] unsigned hends = 0;
	[[maybe_unused]] bool h_any = false, h_simple = false;
	// the two entries of a lane's window that meet a line end when the level's width is a multiple of CPT: column 0 is
	// lane 0's own first column, column W - 1 a lane's own last one (entries 0 and NARR - 1 are never acted on)
	constexpr unsigned kCand = (1u << HK) | (1u << (HK + CPT - 1));
	if constexpr (W::kEndForms) {
		hends = end_mask<NARR>(c0 + lane * CPT - HK, a.W);
		h_any = !a.plain_ends && __builtin_amdgcn_ballot_w64(hends != 0) != 0;
		h_simple = __builtin_amdgcn_ballot_w64((hends & ~(kCand | 1u | (1u << (NARR - 1)))) != 0) == 0;
	}
	// (SelEnds) the same two entries by selection: the lane's flags and its coefficients for the steps that reach them
	[[maybe_unused]] bool e0 = false, e1 = false;
	[[maybe_unused]] T kh[K];
	if constexpr (kIsSelEnds<W>) {
		const unsigned m = end_mask_long<NARR>(c0 + lane * CPT - HK, a.W);
		e0 = (m >> HK) & 1;
		e1 = (m >> (HK + CPT - 1)) & 1;
		sel_coefs<W, false, HK>(kh, e0, e1);
	}
	// (F01) the last column in the middle of a lane's columns (a width that is 4 modulo 8); level 1's candidates in its
	// window of 12 (the neighbours' 4, the lane's own 4): column 0 at entry 4, the last column at 5 or 7, or at 9 -- the
	// right neighbour's second column, which this lane's results reach through step 0; the rows level 1 holds back
	// the lane's phantom LL column (input column pe, window pe - 4 .. pe + 4 at byte `pwin` of a row slot): the last column of
	// the line at entry 5 or 7 of its window, its vertical state and the LL row it holds back
	[[maybe_unused]] bool e1m = false, g0 = false, g5 = false, g7 = false, g9 = false, f5 = false, f7 = false;
	[[maybe_unused]] T st1[K][4] = {}, held[4] = {}, stp[K] = {}, heldp = 0, lop = 0;
	[[maybe_unused]] unsigned pwin = 0;
	[[maybe_unused]] T kp[3] = {}; // the coefficients of entry 5 in steps 0 and 2, of entry 7 in step 0
	if constexpr (F01) {
		e1m = c0 + lane * CPT + 3 == a.W - 1;
		const unsigned m1 = end_mask_long<12>((c0 >> 1) + lane * 4 - 4, a.W >> 1);
		g0 = (m1 >> 4) & 1;
		g5 = (m1 >> 5) & 1;
		g7 = (m1 >> 7) & 1;
		g9 = (m1 >> 9) & 1;
		const int p = lane & 7;
		const int pe = p < 4 ? c0 - 8 + 2 * p : c0 + TW + 2 * (p - 4);
		pwin = (unsigned)(p < 4 ? TW + 2 * p : TW + kHalo + 2 * (p - 4)) * 4;
		const unsigned mp = end_mask_long<9>(pe - 4, a.W);
		f5 = (mp >> 5) & 1;
		f7 = (mp >> 7) & 1;
		kp[0] = f5 ? 2.0f * W::fk(0) : W::fk(0);
		kp[1] = f5 ? 2.0f * W::fk(2) : W::fk(2);
		kp[2] = f7 ? 2.0f * W::fk(0) : W::fk(0);
	}
	// (row_end_test of dwt_sweep2d.h written out, for the same reason)
	// row r (any r the sweep meets) is an end of its column: r == 0 or r == H - 1 after reflection (one bounce when tall)
	[[maybe_unused]] auto row_is_end = [&](int r) {
		if (tall || kIsSelEnds<W>) // (SelEnds runs on levels of 64 rows or more)
			return r == 0 || r == a.H - 1;
		const int rr = reflect(r, a.H);
		return rr == 0 || rr == a.H - 1;
	};

	for (int it = 0; it < kAhead && it < n_iter; it++)
		issue(it);

	for (int it = 0; it < n_iter; it++) {
		if (it + kAhead < n_iter) {
			issue(it + kAhead);
			// everything older than the youngest kAhead iterations' DMAs has landed
			DWT_WAIT_VMCNT(kAhead * kDmaPerIter);
		} else {
			DWT_WAIT_VMCNT(0);
		}

		// horizontal pass of the two rows (2q-1, 2q)
		T row[2][CPT];
		[[maybe_unused]] T xs[2][kPairRows ? NARR : 1];
		// (F01) the lane's phantom column: the windows of both rows, issued ahead of the main columns' reads and complete
		// with them (LDS reads return in order: no wait of their own)
		[[maybe_unused]] u4 pw[2][2];
		[[maybe_unused]] unsigned pw8[2];
		[[maybe_unused]] T rowp[2] = {};
		if constexpr (F01) {
			const unsigned pa = ring_off + (unsigned)rslot * RS * 4 + pwin;
			lds_issue_win9x2(pa, pa + RS * 4, pw[0][0], pw[0][1], pw8[0], pw[1][0], pw[1][1], pw8[1]);
		}
#pragma unroll
		for (int rr = 0; rr < 2; rr++) {
			const unsigned base = ring_off + (unsigned)(rslot + rr) * RS * 4;
			const unsigned own = base + lane * CPT * 4;
			const unsigned la = lane == 0 ? base + (TW + kHaloL) * 4 : own - 16;
			const unsigned ra = lane == 63 ? base + (TW + kHaloR) * 4 : own + CPT * 4;
			T x[NARR];
			u4 L4, R4, O0, O1;
			if constexpr (kShuffle) {
				// own columns from LDS; the tile's outer halo (one 16 B block per side) is
				// read by every lane as a broadcast and used by lanes 0 and 63 only
				u4 H4;
				const unsigned ha = base + TW * 4 + (lane == 63 ? 16 : 0);
				if constexpr (CPT == 8) {
					lds_read2o(own, ha, O0, O1, H4);
				} else {
					lds_read2(own, ha, O0, H4);
					O1 = O0;
				}
#pragma unroll
				for (int e = 0; e < 4; e++) {
					const unsigned l = from_left_lane(O1[e]);  // neighbour's last four columns
					const unsigned r = from_right_lane(O0[e]); // neighbour's first four columns
					L4[e] = lane == 0 ? H4[e] : l;
					R4[e] = lane == 63 ? H4[e] : r;
				}
				if constexpr (CPT == 8) {
#pragma unroll
					for (int e = 0; e < 4; e++)
						x[HK + 4 + e] = from_bits<T>(O1[e]);
				}
			} else if constexpr (CPT == 8) {
				lds_read4(la, own, ra, L4, O0, O1, R4);
#pragma unroll
				for (int e = 0; e < 4; e++)
					x[HK + 4 + e] = from_bits<T>(O1[e]);
			} else {
				lds_read3(la, own, ra, L4, O0, R4);
			}
#pragma unroll
			for (int e = 0; e < HK; e++) {
				x[e] = from_bits<T>(L4[4 - HK + e]);
				x[HK + CPT + e] = from_bits<T>(R4[e]);
			}
#pragma unroll
			for (int e = 0; e < 4; e++)
				x[HK + e] = from_bits<T>(O0[e]);
			if constexpr (kPairRows) {
#pragma unroll
				for (int j = 0; j < NARR; j++)
					xs[rr][j] = x[j];
				continue; // (both rows are lifted together below)
			}
			if constexpr (W::kEndForms) {
				if (__builtin_expect(!h_any, 1)) {
					lift_fwd_regs<W, NARR>(x, 0u);
				} else if (h_simple) {
					DWT_END_PATH();
					lift_fwd_regs<W, NARR, kCand>(x, hends);
				} else {
					DWT_END_PATH();
					lift_fwd_regs<W, NARR>(x, hends);
				}
			} else if constexpr (kIsSelEnds<W>) {
				lift_regs_sel<W, NARR, false, HK, HK + CPT - 1>(x, e0, e1, kh);
			} else {
				lift_fwd_regs<W, NARR>(x, 0u);
			}
#pragma unroll
			for (int v = 0; v < CPT; v++)
				row[rr][v] = W::fwd_scale(v & 1, x[HK + v]);
		}

		if constexpr (kPairRows) {
			// both rows at once, as the halves of packed operations: the same steps, the same rounding (the compiler pairs
			// within a row on its own, but not all of it, and the selects at the two candidate entries split its pairs)
			typedef float f2 __attribute__((ext_vector_type(2)));
			if constexpr (F01) {
				// the phantom column: the four steps on the shrinking window as the main columns take them (entries 5 and 7 by
				// selection, coefficients kp), the scale
				const f2 nz = f2{-0.0f, -0.0f};
				lds_arrived_win9x2(pw[0][0], pw[0][1], pw8[0], pw[1][0], pw[1][1], pw8[1]);
				f2 w2[9];
#pragma unroll
				for (int j = 0; j < 8; j++)
					w2[j] = f2{from_bits<T>(pw[0][j >> 2][j & 3]), from_bits<T>(pw[1][j >> 2][j & 3])};
				w2[8] = f2{from_bits<T>(pw8[0]), from_bits<T>(pw8[1])};
#pragma unroll
				for (int s_ = 0; s_ < K; s_++) {
#pragma unroll
					for (int j = s_ + 1; j <= 7 - s_; j += 2) {
						if (j == 5)
							w2[j] = w2[j] + kp[s_ >> 1] * (w2[j - 1] + (f5 ? nz : w2[j + 1]));
						else if (j == 7)
							w2[j] = w2[j] + kp[2] * (w2[j - 1] + (f7 ? nz : w2[j + 1]));
						else
							w2[j] = w2[j] + W::fk(s_) * (w2[j - 1] + w2[j + 1]);
					}
				}
				const f2 sc = w2[4] * W::fwd_scale(0, 1.0f);
				rowp[0] = sc[0];
				rowp[1] = sc[1];
			}
			f2 x2[NARR];
#pragma unroll
			for (int j = 0; j < NARR; j++)
				x2[j] = f2{xs[0][j], xs[1][j]};
#pragma unroll
			for (int s_ = 0; s_ < K; s_++) {
#pragma unroll
				for (int j = s_ + 1; j <= NARR - 2 - s_; j += 2) {
					if (j == HK)
						x2[j] = x2[j] + kh[s_] * ((e0 ? f2{-0.0f, -0.0f} : x2[j - 1]) + x2[j + 1]);
					else if (j == HK + CPT - 1)
						x2[j] = x2[j] + kh[s_] * (x2[j - 1] + (e1 ? f2{-0.0f, -0.0f} : x2[j + 1]));
					else if (F01 && j == HK + 3)
						x2[j] = x2[j] + (e1m ? 2.0f * W::fk(s_) : W::fk(s_)) * (x2[j - 1] + (e1m ? f2{-0.0f, -0.0f} : x2[j + 1]));
					else
						x2[j] = x2[j] + W::fk(s_) * (x2[j - 1] + x2[j + 1]);
				}
			}
			const float ze = W::fwd_scale(0, 1.0f), zo = W::fwd_scale(1, 1.0f); // (the scale factors themselves)
#pragma unroll
			for (int v = 0; v < CPT; v++) {
				const f2 sc = x2[HK + v] * ((v & 1) ? zo : ze);
				row[0][v] = sc[0];
				row[1][v] = sc[1];
			}
		}
		rslot = rslot + 2 >= kRing ? 0 : rslot + 2;

		// vertical pass: streaming lifting, state in registers
		// step s of this iteration acts on row 2q-1-s: which of them are column ends (wave-uniform; almost never any)
		[[maybe_unused]] bool vend[K] = {};
		[[maybe_unused]] bool v_any = false;
		if constexpr (W::kEndForms) {
#pragma unroll
			for (int s_ = 0; s_ < K; s_++) {
				vend[s_] = row_is_end(2 * (q0 + it) - 1 - s_);
				v_any = !a.plain_ends && (v_any || vend[s_]);
			}
		}
		T lo[CPT], hi[CPT];
		// (fwd_vertical; the policies whose rows are lifted in pairs take two columns at once too -- but for a policy of one
		// step: the scalar form keeps the state in registers)
		auto vertical = [&](auto mode) {
			if constexpr (kPairRows && K != 1) {
				static_assert(decltype(mode)::value == kColNone, "the paired pass has no explicit end forms");
				vertical_pairs<W, CPT>(row, st, lo, hi);
			} else
				fwd_vertical<W, decltype(mode)::value>(row, st, lo, hi, vend);
		};
		if constexpr (W::kEndForms) {
			if (__builtin_expect(v_any, 0)) {
				DWT_END_PATH();
				vertical(ColTag<kColEnds>{});
			}
			else
				vertical(ColTag<kColNone>{});
		} else if constexpr (kIsSelEnds<W>) {
			// step s acts on row 2q-1-s (an upward tile: 2q+1+s); where that row is an end of its column (wave-uniform, the top
			// and bottom tiles' first / last iterations) the step's coefficient is doubled and its state tap -- the same values as
			// the other tap there, in either direction -- gives way to -0.0.  Deep ring: the iterations that meet no end take the plain body.
			bool ve[K], any = false;
#pragma unroll
			for (int s_ = 0; s_ < K; s_++) {
				if constexpr (F01)
					ve[s_] = row_is_end(row_of_step(it, s_));
				else
					ve[s_] = row_is_end(2 * (q0 + it) - 1 - s_);
				any = any || ve[s_];
			}
			// (F01) the phantom column's pass: the main columns' steps on its one column, in the form they take this iteration
			[[maybe_unused]] auto vertical_phantom = [&](auto sel, const T *kv) {
				if constexpr (F01) {
					T n[K + 1];
					n[0] = rowp[1];
#pragma unroll
					for (int s_ = 0; s_ < K; s_++) {
						const bool e = decltype(sel)::value && ve[s_];
						n[s_ + 1] = (s_ ? stp[s_ - 1] : rowp[0]) + (decltype(sel)::value ? kv[s_] : W::fk(s_)) * ((e ? T(-0.0) : stp[s_]) + n[s_]);
					}
					lop = n[K] * W::fwd_scale(0, 1.0f);
#pragma unroll
					for (int s_ = 0; s_ < K; s_++)
						stp[s_] = n[s_];
				}
			};
			auto vertical_sel = [&]() {
				T kv[K];
#pragma unroll
				for (int s_ = 0; s_ < K; s_++)
					kv[s_] = sel_coef<W, false>(s_, ve[s_]);
				if constexpr (F01)
					vertical_phantom(std::true_type{}, kv);
				if constexpr (kPairRows && K != 1)
					vertical_pairs<W, CPT, true>(row, st, lo, hi, ve, kv);
				else
					fwd_vertical<W, kColSel>(row, st, lo, hi, ve, kv);
			};
			// (shallow ring: the launches of a few rounds of waves, bound by the longest wave -- the top tiles', for whom a
			// second body means instructions fetched cold from HBM, 1 us a launch; there every iteration selects)
			if constexpr (SELV && has_coef_ends<W>::value)
				vertical_sel();
			else if (__builtin_expect(any, 0)) {
				DWT_END_PATH();
				vertical_sel();
			} else {
				vertical(ColTag<kColNone>{});
				if constexpr (F01)
					vertical_phantom(std::false_type{}, nullptr);
			}
		} else {
			vertical(ColTag<kColNone>{});
		}

		if constexpr (IL) {
			if (it >= K && (!X || A + it - K >= kIlKeepTop / 2) && a.out_step > 1) {
				// the level goes straight to the lattice it lives on in a larger image: a dword per sample.  Where a
				// deeper level follows, the lattice points at (even row, even column) are its to fill
				const int k = A + it - K;
				const unsigned sb = (unsigned)a.out_step * 4;
				const unsigned cb = (unsigned)(c0 + lane * CPT) * sb;
				const unsigned row_bytes = (unsigned)((X ? a.W - kIlKeepRight : a.W) - 1) * sb + 4;
				const T *r0 = out_h + (long)(2 * k) * a.h_pitch;
				const row_rsrc_t d0 = row_rsrc(r0, row_bytes);
#pragma unroll
				for (int e = 0; e < CPT; e++)
					if ((e & 1) || !a.il_ll)
						store4_row<false>(d0, cb + e * sb, to_bits(lo[e]));
				if (2 * k + 1 < a.H) {
					const row_rsrc_t d1 = row_rsrc(r0 + a.h_pitch, row_bytes);
#pragma unroll
					for (int e = 0; e < CPT; e++)
						store4_row<false>(d1, cb + e * sb, to_bits(hi[e]));
				}
				if (a.il_ll) {
					const row_rsrc_t dl = row_rsrc(out_ll + (long)k * a.ll_pitch, (unsigned)(X ? (a.W - kIlKeepRight + 1) >> 1 : Wd) * 4);
#pragma unroll
					for (int e = 0; e < CPT; e += 4)
						store8_row<false>(dl, (unsigned)(c0 + lane * CPT) * 2 + e * 2, u2{to_bits(lo[e]), to_bits(lo[e + 2])});
				}
			} else
			if (it >= K && (!X || A + it - K >= kIlKeepTop / 2)) {
				const int k = A + it - K;
				const unsigned cb = (unsigned)(c0 + lane * CPT) * 4; // byte offset in an interleaved row
				const T *r0 = out_h + (long)(2 * k) * a.h_pitch;
				// (X: the rows end 8 columns early -- the buffer drops what lies beyond)
				const unsigned row_bytes = (unsigned)(X ? a.W - kIlKeepRight : a.W) * 4;
				const row_rsrc_t d0 = row_rsrc(r0, row_bytes);
				// multi-level: the compose pass reads this (even) row again soon -- temporal, so that it can stay in the
				// Infinity Cache; the odd rows are final: non-temporal
#pragma unroll
				for (int e = 0; e < CPT; e += 4) {
					const u4 v4{to_bits(lo[e]), to_bits(lo[e + 1]), to_bits(lo[e + 2]), to_bits(lo[e + 3])};
					if (a.il_ll == 2)
						store16_row<false>(d0, cb + e * 4, v4);
					else
						store16_row<kNtStore>(d0, cb + e * 4, v4);
				}
				if (2 * k + 1 < a.H) {
					const row_rsrc_t d1 = row_rsrc(r0 + a.h_pitch, row_bytes);
#pragma unroll
					for (int e = 0; e < CPT; e += 4)
						store16_row<kNtStore>(d1, cb + e * 4, u4{to_bits(hi[e]), to_bits(hi[e + 1]), to_bits(hi[e + 2]), to_bits(hi[e + 3])});
				}
				// multi-level: the next level's input (even row, even column) also goes
				// out densely, so that no level has to gather a strided lattice
				if (a.il_ll) {
					const row_rsrc_t dl = row_rsrc(out_ll + (long)k * a.ll_pitch, (unsigned)(X ? (a.W - kIlKeepRight + 1) >> 1 : Wd) * 4);
#pragma unroll
					for (int e = 0; e < CPT; e += 4)
						store8_row<false>(dl, cb / 2 + e * 2, u2{to_bits(lo[e]), to_bits(lo[e + 2])});
				}
			}
		} else
		if constexpr (F01) {
			typedef float f2 __attribute__((ext_vector_type(2)));
			const f2 nz = f2{-0.0f, -0.0f};
			// the pair of level 0 whose L row this iteration completes (downward q - 2, upward q + 2), and the one whose H row
			// (downward the same pair, upward the pair below: q + 1)
			const int k = q0 + dir * (it - K / 2), kh_ = k - up;
			const unsigned clb = (unsigned)((c0 + lane * CPT) >> 1) * 4;
			const unsigned nb0 = (unsigned)Wd * 4;
			if (k >= A && k < B) {
				const T *top = out_h + (long)k * a.h_pitch;
				store16_row<kNtStore>(row_rsrc(top + Wd, nb0), clb, u4{to_bits(lo[1]), to_bits(lo[3]), to_bits(lo[5]), to_bits(lo[7])});
			}
			if (kh_ >= A && kh_ < B) {
				const T *bot = out_h + (long)(Hd + kh_) * a.h_pitch;
				store16_row<kNtStore>(row_rsrc(bot, nb0), clb, u4{to_bits(hi[0]), to_bits(hi[2]), to_bits(hi[4]), to_bits(hi[6])});
				store16_row<kNtStore>(row_rsrc(bot + Wd, nb0), clb, u4{to_bits(hi[1]), to_bits(hi[3]), to_bits(hi[5]), to_bits(hi[7])});
			}
			if (k & 1) {
				// LL row k, odd: waits for its pair
#pragma unroll
				for (int e = 0; e < 4; e++)
					held[e] = lo[2 * e];
				heldp = lop;
			} else {
				// level 1, iteration q1: its rows 2 q1 - 1 (held; an upward tile: 2 q1 + 1) and 2 q1 (this LL row), as the halves of
				// packed operations
				const int q1 = k >> 1, W1 = Wd, H1 = Hd;
				f2 y[12];
				const unsigned pb0 = to_bits(heldp), pb1 = to_bits(lop);
#pragma unroll
				for (int e = 0; e < 4; e++) {
					const unsigned b0 = to_bits(held[e]), b1 = to_bits(lo[2 * e]);
					// (lanes 0 and 63: the phantom columns -- lane e of the lane's quad holds the e-th left one in lanes 0..3, the e-th
					// right one in lanes 60..63: one quad broadcast serves both.  It goes in as the shift's `old` operand, not through
					// a select on the lane: the compiler turns such a select into a branch and runs the shift with the lane masked
					// out, which then no longer serves its neighbour as a source)
					const unsigned q0e = quad_lane(pb0, e), q1e = quad_lane(pb1, e);
					y[e] = f2{from_bits<T>(from_left_lane(b0, q0e)), from_bits<T>(from_left_lane(b1, q1e))};
					y[4 + e] = f2{held[e], lo[2 * e]};
					y[8 + e] = f2{from_bits<T>(from_right_lane(b0, q0e)), from_bits<T>(from_right_lane(b1, q1e))};
				}
#pragma unroll
				for (int s_ = 0; s_ < K; s_++) {
#pragma unroll
					for (int j = s_ + 1; j <= 10 - s_; j += 2) {
						if (j == 4 || j == 5 || j == 7 || j == 9) {
							const bool el = j == 4 && g0, er = j == 5 ? g5 : j == 7 ? g7 : j == 9 ? g9 : false;
							y[j] = y[j] + ((el || er) ? 2.0f * W::fk(s_) : W::fk(s_)) * ((el ? nz : y[j - 1]) + (er ? nz : y[j + 1]));
						} else
							y[j] = y[j] + W::fk(s_) * (y[j - 1] + y[j + 1]);
					}
				}
				const float ze = W::fwd_scale(0, 1.0f), zo = W::fwd_scale(1, 1.0f);
				// vertical pass: step s acts on row 2 q1 - 1 - s (upward: 2 q1 + 1 + s).  An end row drops the tap that lies beyond the
				// band -- what the sweep computes there mirrors level 0's input, not the band --: the end the march meets first
				// (downward row 0, upward row H1 - 1) its older tap, the other end its newer one
				bool vt[K], vb[K];
				T kv[K];
				const int r_old = up ? H1 - 1 : 0, r_new = up ? 0 : H1 - 1;
#pragma unroll
				for (int s_ = 0; s_ < K; s_++) {
					vt[s_] = 2 * q1 - dir * (1 + s_) == r_old;
					vb[s_] = 2 * q1 - dir * (1 + s_) == r_new;
					kv[s_] = (vt[s_] || vb[s_]) ? 2.0f * W::fk(s_) : W::fk(s_);
				}
				auto older = [&](int s_, f2 v) { return vt[s_] ? nz : v; };
				auto newer = [&](int s_, f2 v) { return vb[s_] ? nz : v; };
				T lo1[4], hi1[4];
#pragma unroll
				for (int v = 0; v < 2; v++) {
					// (columns v and v + 2: the stores take them as consecutive registers)
					const f2 c0v = y[4 + v] * (v ? zo : ze), c2v = y[6 + v] * (v ? zo : ze);
					const f2 ov = f2{c0v[0], c2v[0]}, ev = f2{c0v[1], c2v[1]};
					f2 s_[K], n_[K];
#pragma unroll
					for (int i = 0; i < K; i++)
						s_[i] = f2{st1[i][v], st1[i][v + 2]};
					n_[0] = ev;
					n_[1] = ov + kv[0] * (older(0, s_[0]) + newer(0, ev));
					n_[2] = s_[0] + kv[1] * (older(1, s_[1]) + newer(1, n_[1]));
					n_[3] = s_[1] + kv[2] * (older(2, s_[2]) + newer(2, n_[2]));
					const f2 s2n = s_[2] + kv[3] * (older(3, s_[3]) + newer(3, n_[3]));
					const f2 l2 = s2n * ze, h2 = n_[3] * zo;
#pragma unroll
					for (int i = 0; i < K; i++) {
						st1[i][v] = n_[i][0];
						st1[i][v + 2] = n_[i][1];
					}
					lo1[v] = l2[0];
					lo1[v + 2] = l2[1];
					hi1[v] = h2[0];
					hi1[v + 2] = h2[1];
				}
				// level 1's Mallat rows in the LL quadrant of level 0: [LL | HL] at row k1, [LH | HH] at row H1 / 2 + k1h (an upward
				// iteration completes the H row of the pair below its L row's, as level 0 does)
				const int k1 = q1 - dir * (K / 2), k1h = k1 - up;
				const int W2 = W1 >> 1, H2 = H1 >> 1;
				const unsigned cb = (unsigned)((c0 >> 2) + lane * 2) * 4, nb = (unsigned)W2 * 4;
				if (k1 >= (A >> 1) && k1 < (B >> 1)) {
					const T *top = out_h + (long)k1 * a.h_pitch;
					store8_row<kNtStoreLL>(row_rsrc(out_ll + (long)k1 * a.ll_pitch, nb), cb, u2{to_bits(lo1[0]), to_bits(lo1[2])});
					store8_row<kNtStore>(row_rsrc(top + W2, nb), cb, u2{to_bits(lo1[1]), to_bits(lo1[3])});
				}
				if (k1h >= (A >> 1) && k1h < (B >> 1)) {
					const T *bot = out_h + (long)(H2 + k1h) * a.h_pitch;
					store8_row<kNtStore>(row_rsrc(bot, nb), cb, u2{to_bits(hi1[0]), to_bits(hi1[2])});
					store8_row<kNtStore>(row_rsrc(bot + W2, nb), cb, u2{to_bits(hi1[1]), to_bits(hi1[3])});
				}
			}
		} else
		if (it >= K) {
			// Mallat rows: [LL (Wd) | HL (W/2)] at row k, [LH | HH] at row Hd + k; each quarter row is a
			// buffer of its own, so the lanes (and dwords) beyond its end are dropped
			const int k = A + it - K;
			const unsigned clb = (unsigned)((c0 + lane * CPT) >> 1) * 4;
			const T *top = out_h + (long)k * a.h_pitch, *bot = out_h + (long)(Hd + k) * a.h_pitch;
			const unsigned nlb = (unsigned)Wd * 4, nhb = (unsigned)(a.W >> 1) * 4;
			const row_rsrc_t dll = row_rsrc(out_ll + (long)k * a.ll_pitch, nlb), dhl = row_rsrc(top + Wd, nhb);
			const bool hrow = k < (a.H >> 1);
			if constexpr (CPT == 8) {
				store16_row<kNtStoreLL>(dll, clb, u4{to_bits(lo[0]), to_bits(lo[2]), to_bits(lo[4]), to_bits(lo[6])});
				store16_row<kNtStore>(dhl, clb, u4{to_bits(lo[1]), to_bits(lo[3]), to_bits(lo[5]), to_bits(lo[7])});
				if (hrow) {
					store16_row<kNtStore>(row_rsrc(bot, nlb), clb, u4{to_bits(hi[0]), to_bits(hi[2]), to_bits(hi[4]), to_bits(hi[6])});
					store16_row<kNtStore>(row_rsrc(bot + Wd, nhb), clb, u4{to_bits(hi[1]), to_bits(hi[3]), to_bits(hi[5]), to_bits(hi[7])});
				}
			} else {
				store8_row<kNtStoreLL>(dll, clb, u2{to_bits(lo[0]), to_bits(lo[2])});
				store8_row<kNtStore>(dhl, clb, u2{to_bits(lo[1]), to_bits(lo[3])});
				if (hrow) {
					store8_row<kNtStore>(row_rsrc(bot, nlb), clb, u2{to_bits(hi[0]), to_bits(hi[2])});
					store8_row<kNtStore>(row_rsrc(bot + Wd, nhb), clb, u2{to_bits(hi[1]), to_bits(hi[3])});
				}
			}
		}
	}
}

// the tile by the instantiation of the policy's line ends the level needs (dwt_lift.h)
template <class W, int CPT, int RING, int NT, bool IL, bool X>
static __device__ __forceinline__ void fwd_sweep_any_tile(const FwdLevelArgs &a, const SweepGeom &g)
{
	if constexpr (W::kEndForms) {
		if (a.plain_ends)
			fwd_sweep_tile<PlainEnds<W>, CPT, RING, NT, IL, X>(a, g);
		else if (a.W % CPT == 0 && a.W >= 64 && a.H >= 64)
			fwd_sweep_tile<SelEnds<W>, CPT, RING, NT, IL, X>(a, g);
		else // (a width that puts the last column anywhere in a lane's window; short lines, reflected more than once)
			fwd_sweep_tile<W, CPT, RING, NT, IL, X>(a, g);
	} else
		fwd_sweep_tile<W, CPT, RING, NT, IL, X>(a, g);
}

template <class W, int CPT, int RING, int NT, bool IL = false>
__global__ __launch_bounds__(256) void k_fwd_sweep(FwdLevelArgs a, SweepGeom g)
{
	fwd_sweep_any_tile<W, CPT, RING, NT, IL, false>(a, g);
}

// levels 0 and 1 of a float 9/7 transform in one sweep (fwd_sweep_tile, F01).  RING: the ring rows of a wave -- 16: one
// workgroup of four waves per CU, one wave per SIMD; 8: built for two such workgroups per CU, two waves per SIMD
template <int NT, int RING = 16>
__global__ __launch_bounds__(256, RING == 16 ? 1 : 2) void k_fwd_sweep01(FwdLevelArgs a, SweepGeom g, int updown)
{
	fwd_sweep_tile<SelEnds<Cdf97S>, 8, RING, NT, false, false, true, false>(a, g, updown);
}

// a level with a rectangle copy riding along: the workgroups behind the tiles' copy blocks of `r` (FwdLevelArgs::ride)
template <class W, int CPT, int RING, int NT>
__global__ __launch_bounds__(256) void k_fwd_sweep_r(FwdLevelArgs a, SweepGeom g, CopyRects r)
{
	if ((int)blockIdx.x >= g.tile_blocks) {
		ride_copy_block(r, (int)blockIdx.x - g.tile_blocks);
		return;
	}
	fwd_sweep_any_tile<W, CPT, RING, NT, false, false>(a, g);
}

// one level of a phase-ordered interleaved transform, exact: workgroups [0, g.first) compute the border strips
template <class W, int CPT, int RING, int NT>
__global__ __launch_bounds__(256) void k_fwd_sweep_x(FwdLevelArgs a, SweepGeom g, IlStripArgs strip)
{
	if ((int)blockIdx.x < g.first) {
		il_strip_wave<W, false>(strip, blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
		return;
	}
	fwd_sweep_any_tile<W, CPT, RING, NT, true, true>(a, g);
}

// ---- launch wrappers -------------------------------------------------------------
template <class W, int CPT, int RING, int NT, bool IL = false>
static hipError_t fwd_launch(const FwdLevelArgs &a, const SweepGeom &g, dim3 grid, int waves, hipStream_t s)
{
	const size_t lds = (size_t)waves * RING * (64 * CPT + 8) * 4;
	if constexpr (!IL && RING == 8 && (NT == 7 || NT == 3)) {
		// (the variants a level of one image takes; the launcher has checked batch == 1 and four waves)
		if (a.ride && a.ride_hi > a.ride_lo) {
			if (hipError_t e = allow_lds((const void *)k_fwd_sweep_r<W, CPT, RING, NT>, lds))
				return e;
			SweepGeom gr = g;
			gr.tile_blocks = (int)grid.x;
			CopyRects r = *a.ride;
			r.block0 = a.ride_lo;
			k_fwd_sweep_r<W, CPT, RING, NT><<<dim3(grid.x + (unsigned)(a.ride_hi - a.ride_lo), 1), 64 * waves, lds, s>>>(a, gr, r);
			return hipGetLastError();
		}
	}
	if (a.ride && a.ride_hi > a.ride_lo)
		return hipErrorInvalidValue; // the caller asked for a variant that has no ride-along kernel
	if (hipError_t e = allow_lds((const void *)k_fwd_sweep<W, CPT, RING, NT, IL>, lds))
		return e;
	k_fwd_sweep<W, CPT, RING, NT, IL><<<grid, 64 * waves, lds, s>>>(a, g);
	return hipGetLastError();
}

template <class W, int CPT>
static hipError_t fwd_pick(const FwdLevelArgs &a, const SweepGeom &g, dim3 grid, int waves, const SweepTuning &t, hipStream_t s)
{
	// cache policy 6 (non-temporal loads, every store temporal: the staged outputs of an in-place call, read back
	// at once), 7 (non-temporal loads and detail stores, the LL band's stores temporal), 3 (the LL band
	// non-temporal too: launches whose LL bands exceed the Infinity Cache), 15 (= 7 with the neighbour taps
	// by wavefront shifts instead of LDS reads: bit-identical, 0.8 % slower, the cross-check variant).  The
	// other policies and ring depths of rounds 1-3 measured slower and are gone (profiles/archive/r02_experiments.md).
	const int nt = a.temporal ? 6 : (t.nt & 8) ? 15 : (t.nt & 4) ? 7 : 3;
	if (t.ring == 16) {
		switch (nt) {
		case 6: return fwd_launch<W, CPT, 16, 6>(a, g, grid, waves, s);
		case 3: return fwd_launch<W, CPT, 16, 3>(a, g, grid, waves, s);
		case 7: return fwd_launch<W, CPT, 16, 7>(a, g, grid, waves, s);
		default: return fwd_launch<W, CPT, 16, 15>(a, g, grid, waves, s);
		}
	}
	switch (nt) {
	case 6: return fwd_launch<W, CPT, 8, 6>(a, g, grid, waves, s);
	case 3: return fwd_launch<W, CPT, 8, 3>(a, g, grid, waves, s);
	case 7: return fwd_launch<W, CPT, 8, 7>(a, g, grid, waves, s);
	default: return fwd_launch<W, CPT, 8, 15>(a, g, grid, waves, s);
	}
}

template <class W, int RING>
static hipError_t fwd_launch_x(const FwdLevelArgs &a, SweepGeom g, dim3 grid, int waves, const IlStripArgs &strip, hipStream_t s)
{
	const size_t lds = (size_t)waves * RING * (64 * 4 + 8) * 4;
	if (hipError_t e = allow_lds((const void *)k_fwd_sweep_x<W, 4, RING, 3>, lds))
		return e;
	g.first = il_strip_blocks(a.W, a.H, waves);
	grid.x += g.first;
	k_fwd_sweep_x<W, 4, RING, 3><<<grid, 64 * waves, lds, s>>>(a, g, strip);
	return hipGetLastError();
}

template <class W>
static hipError_t fwd_level_t(const FwdLevelArgs &a, const SweepTuning &t, hipStream_t s, const IlStripArgs *strip = nullptr)
{
	if (a.W < 2 || a.H < 2 || a.batch < 1)
		return hipErrorInvalidValue;
	const int cpt = a.interleaved ? 4 : pick_cpt(t, a.W, false);
	const int TW = 64 * cpt;
	SweepGeom g;
	g.tile_pairs = pick_tile_pairs(t, a.W, a.H, cpt, a.batch);
	g.ntx = (a.W + TW - 1) / TW;
	g.swz = t.xcd_swizzle;
	g.wave_horiz = 0;
	const int Hd = (a.H + 1) / 2;
	const int waves = sweep_waves(t);
	const int nty = (Hd + g.tile_pairs - 1) / g.tile_pairs;
	// Ring depth (measured, scripts/sweep.py): when a launch has several rounds of tiles
	// per CU, 4 waves/CU with a 16-row ring (7 iterations of DMA in flight per wave) and
	// side-by-side waves beat 8 waves/CU with an 8-row ring (5.5 -> 6.0 TB/s at level 0);
	// smaller launches prefer more resident waves.
	SweepTuning tt = t;
	if (tt.ring != 8 && tt.ring != 16)
		// (one image in the interleaved layout: from 512 tiles on -- 8192^2 J=5 250-252 -> 247.5-248 us, the Mallat entry
		// loses 5 us of 148 with that threshold; measured in one process, alternated)
		tt.ring = (g.ntx >= waves && (long)g.ntx * nty * a.batch >= ((a.interleaved && a.batch == 1) ? 512 : 3072)) ? 16 : 8;
	// deep ring: the waves of a workgroup take side-by-side tiles (+ 7 %); shallow: stacked tiles
	g.wave_horiz = tt.ring == 16;
	const dim3 grid = sweep_grid(g, nty, waves, a.batch);
	if (a.sh.rows && (!a.interleaved || a.batch != 1 || a.out_step != 1 || g.tile_pairs != a.sh.tile_pairs))
		return hipErrorInvalidValue; // the snapshot of an in-place level was taken for other tiles
	if (a.ride && a.ride_hi > a.ride_lo && (a.interleaved || a.batch != 1 || waves != 4 || tt.ring != 8 || a.temporal || (tt.nt & 8)))
		return hipErrorInvalidValue; // (fwd_ride_ok says when a copy may ride along)
	if (a.interleaved) {
		// 3-D path: float 9/7 only; always 4 columns per lane so that each row leaves the
		// wave as ONE contiguous 16 B/lane store (two strided stores per row cost 40 %)
		if constexpr (std::is_same<W, Cdf97S>::value || std::is_same<W, Cdf53SNew>::value) {
			// exact border strips in the same launch (one image, levels of 64 samples or more either way)
			if (strip) {
				if (a.batch != 1 || a.W < 64 || a.H < 64)
					return hipErrorInvalidValue;
				return tt.ring == 16 ? fwd_launch_x<W, 16>(a, g, grid, waves, *strip, s) : fwd_launch_x<W, 8>(a, g, grid, waves, *strip, s);
			}
		}
		if (strip)
			return hipErrorInvalidValue;
		if constexpr (std::is_base_of<Cdf97S, W>::value || std::is_base_of<Cdf53S, W>::value) {
			if (tt.ring == 16)
				return fwd_launch<W, 4, 16, 3, true>(a, g, grid, waves, s);
			return fwd_launch<W, 4, 8, 3, true>(a, g, grid, waves, s);
		} else {
			return hipErrorInvalidValue;
		}
	}
	if (strip)
		return hipErrorInvalidValue;
	// Cache policy bit 2 keeps the LL band's stores temporal so that the next level finds it in the
	// 256 MiB Infinity Cache.  The LL bands of a large batch do not fit (64 images of 8192^2: 4.3 GB):
	// temporal stores then only displace other lines -- non-temporal like the detail bands (64 images,
	// one process, alternated: level 0 5863-5882 -> 5959-5964 GB/s, level 1 5323-5341 -> 5381-5409, step
	// 8.08-8.10 -> 8.00-8.02 ms).  At 0.5 GB of LL (8 images) the two policies tie (level 0 loses what
	// level 1 gains), below that temporal wins: switch from 1 GiB on.  Option nt_auto = 0 turns it off.
	if (tt.nt_auto && (tt.nt & 12) == 4 && (size_t)a.batch * ((a.W + 1) / 2) * ((a.H + 1) / 2) * sizeof(typename W::T) >= ((size_t)1 << 30))
		tt.nt = 3;
	return cpt == 8 ? fwd_pick<W, 8>(a, g, grid, waves, tt, s) : fwd_pick<W, 4>(a, g, grid, waves, tt, s);
}

// ---- the fused pair of levels 0 and 1 --------------------------------------------
bool fwd01_can(Wavelet w, int W, int H)
{
	// (both levels of 64 x 64 or more: the select form of the line ends; the build with reflected ends has none)
	return Cdf97S::kEndForms && w == kCdf97S && W % 4 == 0 && H % 4 == 0 && W >= 128 && H >= 128;
}

int fwd01_tiles(int W)
{
	return (W + 511) / 512; // the level-0 sweep's own tiles
}

bool fwd01_has_ring(int ring)
{
	return ring == 16 || ring == 8;
}

// The ring rows of the fused pair's launch: option fuse01_ring or the tuner's choice (SweepTuning::fuse01_ring, never `ring`:
// that one set to 8 keeps a call level by level, pair01_ok), else this rule: 8 rows -- two workgroups per CU, a second wave on
// every SIMD to issue while the first one waits -- in the launches the pair engages in by itself, 32768 tiles of 64 pairs and
// more; 16 rows, as before, below that, where only fuse01 = 2 brings the pair and nothing was measured.  The fused launch of
// the whole 5-level call, 16 against 8 rows, one process, alternated, buffers placed by dwt_hip_alloc_batch: 64 x 8192^2
// 6.77 -> 6.16 ms, 256 x 4096^2 6.81 -> 6.22 ms (the 16-row launches within 0.09 ms of each other); on plain allocations and
// the two levels alone 6.87 -> 6.93 ms (a tie) and 6.99 -> 6.61 ms.  profiles/fuse01_ring_summary.md.
// (the launches the pair engages in by itself: 32768 tiles of 64 pairs and more)
static bool fwd01_large(int W, int H, int batch)
{
	return (long)fwd01_tiles(W) * (((H >> 1) + 63) / 64) * batch >= 32768;
}

static int fwd01_ring(const SweepTuning &t, int W, int H, int batch)
{
	if (t.fuse01_ring)
		return t.fuse01_ring;
	return fwd01_large(W, H, batch) ? 8 : 16;
}

bool fwd01_has_updown(int v)
{
	return v >= -1 && v <= 2;
}

// Which tile rows of the fused pair's launch march upward: option fuse01_updown or the tuner's choice, else this rule: the odd
// ones in the launches of 32768 tiles and more that run the 8-row ring (by the ring's rule or by option fuse01_ring), none in the
// others -- smaller launches, the 16-row ring --, where nothing was measured.  A downward tile and the upward one below it (and the other way round) reach the 22 rows around their common
// edge at the same time, so the second read of those rows -- 17 % of the launch's reads -- hits in L2: the fused launch of
// the whole 5-level call, all downward against odd rows upward, one process, alternated, placed buffers: 64 x 8192^2
// 6.10 -> 6.00 ms, 256 x 4096^2 6.24 -> 5.97 ms (the traffic probe ahead of it: 6.22 -> 6.00 and 6.22 -> 6.12 ms, FETCH_SIZE x 2
// from 1.172 x to 1.050 x the input; profiles/fuse01_updown_summary.md).
int fwd01_updown(const SweepTuning &t, int W, int H, int batch)
{
	if (t.fuse01_updown >= 0)
		return t.fuse01_updown;
	return fwd01_large(W, H, batch) && fwd01_ring(t, W, H, batch) == 8 ? 1 : 0;
}

hipError_t launch_fwd01(const FwdLevelArgs &a, const SweepTuning &t, hipStream_t s)
{
	if (!fwd01_can(kCdf97S, a.W, a.H) || a.batch < 1 || a.interleaved || a.ride || a.pair_hi > 0 || (t.tile_pairs & 1))
		return hipErrorInvalidValue;
	const int ring = fwd01_ring(t, a.W, a.H, a.batch);
	if (!fwd01_has_ring(ring) || !fwd01_has_updown(t.fuse01_updown))
		return hipErrorInvalidValue;
	const int waves = sweep_waves(t);
	const int Hd = a.H >> 1;
	SweepGeom g;
	g.ntx = fwd01_tiles(a.W);
	g.swz = t.xcd_swizzle;
	g.wave_horiz = 1;
	const int updown = fwd01_updown(t, a.W, a.H, a.batch);
	g.tile_pairs = t.tile_pairs;
	if (g.tile_pairs <= 0) {
		// 7 iterations of a tile are level 1's warm-up: tall tiles, unless that leaves too few of them
		g.tile_pairs = 64;
		while (g.tile_pairs > 16 && (long)g.ntx * ((Hd + g.tile_pairs - 1) / g.tile_pairs) * a.batch < 1024)
			g.tile_pairs >>= 1;
	}
	const long tiles = (long)g.ntx * ((Hd + g.tile_pairs - 1) / g.tile_pairs);
	const dim3 grid((unsigned)((tiles + waves - 1) / waves), a.batch);
	// (16 rows: 139 264 B of 160 KiB for four waves, one workgroup per CU, as the level-0 sweep's deep ring; 8 rows: 69 632 B, two
	// workgroups per CU)
	const size_t lds = (size_t)waves * ring * (64 * 8 + 32) * 4;
	// Cache policy as fwd_pick reads `nt`: loads and detail stores non-temporal whatever its bits 0 and 1 say; bit 2 keeps
	// the LL band's stores -- here level 1's -- temporal while the launch's bands fit the Infinity Cache (as fwd_level_t
	// decides it).  Bit 3, the sweep option `ring` = 8 and 4 columns per lane have no fused kernel: pair01_ok keeps such settings
	// level by level; `ring` 16 is what this kernel's tiles are, whatever the depth of its own ring.
	const bool ll_nt = !(t.nt & 4) || (t.nt_auto && (size_t)a.batch * (a.W >> 2) * (a.H >> 2) * sizeof(float) >= ((size_t)1 << 30));
	auto launch = [&](auto k) {
		if (hipError_t e = allow_lds((const void *)k, lds))
			return e;
		k<<<grid, 64 * waves, lds, s>>>(a, g, updown);
		return hipGetLastError();
	};
	if (ring == 16)
		return ll_nt ? launch(k_fwd_sweep01<3, 16>) : launch(k_fwd_sweep01<7, 16>);
	return ll_nt ? launch(k_fwd_sweep01<3, 8>) : launch(k_fwd_sweep01<7, 8>);
}

// whether launch_fwd_level / launch_inv_level would take a kernel that can carry a copy along for this level
bool sweep_ride_ok(const SweepTuning &t, int W, int H, int batch, bool inverse)
{
	if (batch != 1 || W < 2 || H < 2 || !(t.waves >= 1 && t.waves <= 4 ? t.waves == 4 : true) || (t.nt & 8))
		return false;
	if (inverse)
		return t.ring_inv != 16;
	if (t.ring == 16)
		return false;
	if (t.ring == 8)
		return true;
	// the launcher's own ring choice (fwd_level_t): the deep ring from 3072 tiles on
	const int cpt = pick_cpt(t, W, false);
	const int tp = pick_tile_pairs(t, W, H, cpt, 1);
	const long ntx = (W + 64 * cpt - 1) / (64 * cpt), nty = ((H + 1) / 2 + tp - 1) / tp;
	return !(ntx >= 4 && ntx * nty >= 3072);
}

int il_sweep_tile_pairs(const SweepTuning &t, int W, int H, bool inverse)
{
	return pick_tile_pairs(t, W, H, 4, 1, inverse, true);
}

hipError_t launch_fwd_level(Wavelet w, const FwdLevelArgs &a, const SweepTuning &t, hipStream_t s, const IlStripArgs *strip)
{
	if (strip && w != kCdf97S && w != kCdf53SNew)
		return hipErrorInvalidValue;
	switch (w) {
	case kCdf97S: return fwd_level_t<Cdf97S>(a, t, s, strip);
	case kCdf53I: return fwd_level_t<Cdf53I>(a, t, s);
	case kCdf53S: return fwd_level_t<Cdf53S>(a, t, s);
	case kCdf97I: return fwd_level_t<Cdf97I>(a, t, s);
	case kCdf97SFma: return fwd_level_t<Cdf97SFma>(a, t, s);
	case kCdf53SNew: return a.interleaved ? fwd_level_t<Cdf53SNew>(a, t, s, strip) : hipErrorInvalidValue;
	case kInterp53S: return a.interleaved ? hipErrorInvalidValue : fwd_level_t<Interp53S>(a, t, s);
	default: break; // the double-precision drivers run on the line-pass kernels
	}
	return hipErrorInvalidValue;
}

} // namespace dwt
