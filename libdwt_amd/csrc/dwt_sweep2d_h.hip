// dwt_sweep2d_h.hip -- the fused tile sweeps of the float CDF 9/7 on binary16 storage (Cdf97H, dwt_lift.h):
// one launch per level of a dense Mallat frame or batch, every sample read once and every coefficient written once --
// and the two frame conversions of the line-pass route.
//
// It sits beside dwt_sweep2d_i16.hip: the tile origin, the streaming vertical pass and the grid are the shared pieces of
// dwt_sweep2d.h, rows go straight to registers (no LDS ring), the rows of the next two iterations being fetched while this
// one's are lifted, and nothing is read or written outside the W x H region of an image.  What differs from the int16 sweeps:
//
//   - ORDER.  Rows, then columns, both ways, as the float sweeps: the horizontal lift of the two rows of an iteration in
//     registers -- both rows at once, as the halves of packed binary32 operations --, then the streaming vertical pass on
//     the lane's own columns (no halo column is lifted vertically).
//   - ARITHMETIC in binary32.  Samples are widened on load (exact) and the level's results narrowed on store, round to
//     nearest even, once; the row pass's result never leaves the registers, so it is never rounded to binary16.
//   - HALO of K = 4.  The horizontal lift of a lane's columns c .. c + CPT - 1 reads 4 columns to their left and 3 to their
//     right (the inverse: samples c - 3 .. c + CPT + 3).  Lanes whose window lies inside the row fetch the halo as aligned
//     dwords (forward: two 8-byte loads; inverse: three dwords and a sample); lanes at a row's ends, and rows whose
//     subband starts at an odd sample, fetch it sample by sample through reflected indices.
//   - LINE ENDS by reflection: Cdf97H has no end forms (dwt_lift.h says why the bits are the reference's).
//   - ALIGNMENT as in the int16 sweeps: bases, pitches and batch strides are multiples of 4 bytes (call2d), a lane's
//     own bytes of an image row are dword-aligned; the subbands right of the LL / LH quarter start at sample ceil(W/2)
//     and are accessed sample by sample where that is odd (a test on the address, uniform over the wave).
#include "dwt_sweep2d.h"

namespace dwt {

namespace {

typedef u4 u4a __attribute__((aligned(4)));
typedef u2 u2a __attribute__((aligned(4)));
typedef unsigned short hbits; // a binary16 sample as it lies in memory
typedef float f2 __attribute__((ext_vector_type(2)));

// iterations (row pairs) a wave fetches ahead of the one it lifts: the rows wait in registers
constexpr int kAheadH = 2;

static __device__ __forceinline__ bool dword_aligned(const void *p) { return ((uintptr_t)p & 3) == 0; }

// widen / narrow: plain conversions (v_cvt_f32_f16 exact; v_cvt_f16_f32 round to nearest even, overflow to Inf, subnormals kept)
static __device__ __forceinline__ float widen(unsigned bits) { return (float)__builtin_bit_cast(_Float16, (hbits)bits); }
static __device__ __forceinline__ unsigned narrow(float v) { return __builtin_bit_cast(hbits, (_Float16)v); }
// sample i (0 = low half) of a packed pair
static __device__ __forceinline__ float half_of(unsigned w, int i) { return widen(i ? w >> 16 : w & 0xffffu); }
static __device__ __forceinline__ unsigned pack_bits(unsigned lo, unsigned hi) { return (lo & 0xffffu) | (hi << 16); }
static __device__ __forceinline__ unsigned pack_pair(float lo, float hi) { return narrow(lo) | (narrow(hi) << 16); }

// reflection of column / sample index i into a line of N >= 2: one bounce for the lines long enough (i within 20 of
// the line), the general form otherwise
static __device__ __forceinline__ int refl_h(int i, int N)
{
	return N >= 32 ? reflect_near(i, N) : reflect(i, N);
}

// two consecutive samples at p as one dword (p's alignment: uniform over the wave)
static __device__ __forceinline__ unsigned load_pair(const hbits *p)
{
	if (dword_aligned(p))
		return *(const unsigned *)p;
	return pack_bits(p[0], p[1]);
}

// the first n of 2 * ND consecutive samples (packed in v) to p: 16-byte (ND = 2: 8-byte) stores where all are wanted and p is
// dword-aligned
template <bool NT, int ND>
static __device__ __forceinline__ void store_samples(hbits *p, const unsigned (&v)[ND], int n)
{
	static_assert(ND == 2 || ND == 4 || ND == 8, "8, 16 or twice 16 bytes");
	if constexpr (ND == 8) {
		const unsigned a[4] = {v[0], v[1], v[2], v[3]}, b[4] = {v[4], v[5], v[6], v[7]};
		store_samples<NT>(p, a, n);
		store_samples<NT>(p + 8, b, n - 8);
		return;
	} else if (n >= 2 * ND && dword_aligned(p)) {
		if constexpr (ND == 4) {
			const u4a q = {v[0], v[1], v[2], v[3]};
			if constexpr (NT)
				__builtin_nontemporal_store(q, (u4a *)p);
			else
				*(u4a *)p = q;
		} else {
			const u2a q = {v[0], v[1]};
			if constexpr (NT)
				__builtin_nontemporal_store(q, (u2a *)p);
			else
				*(u2a *)p = q;
		}
		return;
	} else {
#pragma unroll
		for (int i = 0; i < 2 * ND; i++)
			if (i < n)
				p[i] = (hbits)((i & 1) ? v[i >> 1] >> 16 : v[i >> 1]);
	}
}

} // namespace

// ---- forward ---------------------------------------------------------------------------
// what a lane fetches of one row: its own CPT columns packed, the columns c - 4 .. c - 1 and c + CPT .. c + CPT + 3
template <int CPT>
struct FwdRawH {
	unsigned m[CPT / 2];
	u2 l, r;
};

template <class W, int CPT>
__global__ __launch_bounds__(256) void k_fwd_sweep_h(FwdLevelArgs a, SweepGeom g)
{
	using T = typename W::T;
	constexpr int K = W::K, TW = 64 * CPT, NARR = CPT + 2 * K - 1;
	static_assert(K == 4 && (CPT == 8 || CPT == 16), "the 9/7 steps; 16 or 32 bytes of a row per lane");

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
	const bool left_in = c >= K, right_in = c + CPT + K <= a.W; // the halo's four samples lie inside the row
	const int n_iter = (B - A) + K;
	const int q0 = A - K / 2;

	const hbits *in = (const hbits *)a.in + (long)img * a.in_bstride;
	hbits *out_ll = (hbits *)a.out_ll + (long)img * a.ll_bstride;
	hbits *out_h = (hbits *)a.out_h + (long)img * a.h_bstride;
	const bool tall = a.H >= 64;

	auto fetch = [&](int it, FwdRawH<CPT> (&raw)[2]) {
#pragma unroll
		for (int rr = 0; rr < 2; rr++) {
			const int ri = 2 * (q0 + it) - 1 + rr;
			const int r = tall ? reflect1(ri, a.H) : reflect(ri, a.H);
			const hbits *grow = in + (long)r * a.in_pitch;
			if (full) {
				// (every row is read once, but for the few around a tile's upper edge)
#pragma unroll
				for (int i = 0; i < CPT / 8; i++) {
					const u4 v = __builtin_nontemporal_load((const u4a *)(grow + c + 8 * i));
					raw[rr].m[4 * i] = v[0];
					raw[rr].m[4 * i + 1] = v[1];
					raw[rr].m[4 * i + 2] = v[2];
					raw[rr].m[4 * i + 3] = v[3];
				}
			} else {
				// the lane overhangs the row's end: its columns one by one, reflected
#pragma unroll
				for (int j = 0; j < CPT; j += 2)
					raw[rr].m[j >> 1] = pack_bits(grow[refl_h(c + j, a.W)], grow[refl_h(c + j + 1, a.W)]);
			}
			if (left_in)
				raw[rr].l = *(const u2a *)(grow + c - K);
			else
				raw[rr].l = u2{pack_bits(grow[refl_h(c - 4, a.W)], grow[refl_h(c - 3, a.W)]), pack_bits(grow[refl_h(c - 2, a.W)], grow[refl_h(c - 1, a.W)])};
			if (right_in)
				raw[rr].r = *(const u2a *)(grow + c + CPT);
			else
				raw[rr].r = u2{pack_bits(grow[refl_h(c + CPT, a.W)], grow[refl_h(c + CPT + 1, a.W)]), pack_bits(grow[refl_h(c + CPT + 2, a.W)], 0)};
		}
	};

	T st[K][CPT];
#pragma unroll
	for (int s = 0; s < K; s++)
#pragma unroll
		for (int v = 0; v < CPT; v++)
			st[s][v] = 0;

	FwdRawH<CPT> q[kAheadH + 1][2]; // q[0]: this iteration's rows
#pragma unroll
	for (int d = 0; d < kAheadH; d++)
		if (d < n_iter)
			fetch(d, q[d]);
	for (int it = 0; it < n_iter; it++) {
		if (it + kAheadH < n_iter)
			fetch(it + kAheadH, q[kAheadH]);
		const FwdRawH<CPT> (&cur)[2] = q[0];
		// rows first: x[j] = column c - 4 + j of the row (x[0] even), the K steps, the lane's columns at x[4 .. 4 + CPT - 1]
		// Both rows at once, as the halves of packed operations: the steps and the rounding of W::fwd_step / fwd_scale (as
		// in the float sweeps: c + k (l + r), multiply and add unfused).
		T row[2][CPT];
		{
			f2 x[NARR];
#pragma unroll
			for (int j = 0; j < K; j++)
				x[j] = f2{half_of(cur[0].l[j >> 1], j & 1), half_of(cur[1].l[j >> 1], j & 1)};
#pragma unroll
			for (int j = 0; j < CPT; j++)
				x[K + j] = f2{half_of(cur[0].m[j >> 1], j & 1), half_of(cur[1].m[j >> 1], j & 1)};
#pragma unroll
			for (int j = 0; j < K - 1; j++)
				x[K + CPT + j] = f2{half_of(cur[0].r[j >> 1], j & 1), half_of(cur[1].r[j >> 1], j & 1)};
#pragma unroll
			for (int s = 0; s < K; s++) {
#pragma unroll
				for (int j = s + 1; j <= NARR - 2 - s; j += 2)
					x[j] = x[j] + W::fk(s) * (x[j - 1] + x[j + 1]);
			}
			const float ze = W::fwd_scale(0, 1.0f), zo = W::fwd_scale(1, 1.0f); // (the scale factors themselves)
#pragma unroll
			for (int v = 0; v < CPT; v++) {
				const f2 sc = x[K + v] * ((v & 1) ? zo : ze);
				row[0][v] = sc[0];
				row[1][v] = sc[1];
			}
		}
		// then the columns, two at once (reflected rows: the policy has no end forms)
		T lo[CPT], hi[CPT];
		vertical_pairs<W, CPT>(row, st, lo, hi);
		if (it >= K) {
			const int k = A + it - K;
			// the level's only rounding: each subband's CPT / 2 samples of the row, narrowed and packed
			unsigned ll[CPT / 4], hl[CPT / 4], lh[CPT / 4], hh[CPT / 4];
#pragma unroll
			for (int i = 0; i < CPT / 4; i++) {
				ll[i] = pack_pair(lo[4 * i], lo[4 * i + 2]);
				hl[i] = pack_pair(lo[4 * i + 1], lo[4 * i + 3]);
				lh[i] = pack_pair(hi[4 * i], hi[4 * i + 2]);
				hh[i] = pack_pair(hi[4 * i + 1], hi[4 * i + 3]);
			}
			const int cl = c >> 1;
			const int nl = Wd - cl, nh = (a.W >> 1) - cl; // samples left in the L / H half from the lane's first
			hbits *top = out_h + (long)k * a.h_pitch, *bot = out_h + (long)(Hd + k) * a.h_pitch;
			store_samples<false>(out_ll + (long)k * a.ll_pitch + cl, ll, nl); // the next level reads it: temporal
			store_samples<true>(top + Wd + cl, hl, nh);
			if (k < (a.H >> 1)) {
				store_samples<true>(bot + cl, lh, nl);
				store_samples<true>(bot + Wd + cl, hh, nh);
			}
		}
#pragma unroll
		for (int d = 0; d < kAheadH; d++) {
			q[d][0] = q[d + 1][0];
			q[d][1] = q[d + 1][1];
		}
	}
}

static int h_tile_pairs(const SweepTuning &t, long ntx, int Hd, long samples, int batch, int big, long want)
{
	if (t.tile_pairs > 0)
		return t.tile_pairs;
	// tile heights as the int16 sweeps pick them (the same bytes per row): small levels are one round of waves and want
	// short tiles, large ones tall tiles (the K-row warm-up re-reads the tile above)
	if (samples <= (2L << 20))
		return 2;
	if (samples <= (8L << 20))
		return 4;
	int tp = big;
	while (tp > 8 && ntx * ((Hd + tp - 1) / tp) * batch < want)
		tp >>= 1;
	return tp;
}

// Columns per lane.  The library builds 8 only.  The templates also compile at 16 (the CPT / 8 load loop, the ND == 8 branch
// of store_samples): that width is never instantiated here and is kept so that the compiler's resource report of both
// widths can be made again by changing these two constants.
constexpr int kFwdCptH = 8, kInvCptH = 8;

hipError_t launch_fwd_level_h(Wavelet w, const FwdLevelArgs &a, const SweepTuning &t, hipStream_t s)
{
	if (w != kCdf97H || a.W < 2 || a.H < 2 || a.batch < 1 || a.interleaved)
		return hipErrorInvalidValue;
	constexpr int TW = 64 * kFwdCptH;
	SweepGeom g;
	const int Hd = (a.H + 1) / 2;
	g.ntx = (a.W + TW - 1) / TW;
	g.tile_pairs = h_tile_pairs(t, g.ntx, Hd, (long)a.W * a.H * a.batch, a.batch, 64, 2048);
	g.swz = t.xcd_swizzle;
	g.wave_horiz = 0; // stacked tiles
	const int waves = sweep_waves(t);
	const dim3 grid = sweep_grid(g, (Hd + g.tile_pairs - 1) / g.tile_pairs, waves, a.batch);
	k_fwd_sweep_h<Cdf97H, kFwdCptH><<<grid, 64 * waves, 0, s>>>(a, g);
	return hipGetLastError();
}

// ---- inverse ---------------------------------------------------------------------------
// A lane owns CPT output columns c .. c + CPT - 1 (one store per row).  Source rows are Mallat rows: "L row p" = [LL | HL],
// "H row p" = [LH | HH]; interleaved sample i of a row is L[i / 2] for even i and H[i / 2] for odd i.  The horizontal
// inverse of the lane's columns reads the samples c - 3 .. c + CPT + 3: with cl = c / 2 and n = CPT / 2 its own L[cl .. cl + n)
// and H[cl .. cl + n), and the halo H[cl - 2], H[cl - 1] (hl), L[cl - 1] (ll), L[cl + n], L[cl + n + 1] (lr), H[cl + n], H[cl + n + 1] (hr).
template <int CPT>
struct InvRawH {
	unsigned l[CPT / 4], h[CPT / 4];
	unsigned hl, ll, lr, hr;
};

template <class W, int CPT>
__global__ __launch_bounds__(256) void k_inv_sweep_h(InvLevelArgs a, SweepGeom g)
{
	using T = typename W::T;
	constexpr int K = W::K, TW = 64 * CPT, NARR = CPT + 2 * K - 1, NS = CPT / 2;
	static_assert(K == 4 && (CPT == 8 || CPT == 16), "the 9/7 steps; 16 or 32 bytes of a row per lane");

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
	const bool inside = c >= K - 1 && c + CPT + K - 1 < a.W; // the samples c - 3 .. c + CPT + 3 lie inside the row
	const int cl = c >> 1;
	const int n_iter = (B - A) + K;
	const int p0 = A - K / 2;

	const hbits *in_ll = (const hbits *)a.in_ll + (long)img * a.ll_bstride;
	const hbits *in_h = (const hbits *)a.in_h + (long)img * a.h_bstride;
	hbits *out = (hbits *)a.out + (long)img * a.out_bstride;
	const bool tall = a.H >= 64;

	auto fetch = [&](int it, InvRawH<CPT> (&raw)[2]) {
		const int p = p0 + it;
#pragma unroll
		for (int rr = 0; rr < 2; rr++) {
			const int rs = tall ? reflect1(2 * p + rr, a.H) : reflect(2 * p + rr, a.H);
			const int sub = rs >> 1;
			const hbits *gl, *gh;
			if ((rs & 1) == 0) {
				gl = in_ll + (long)sub * a.ll_pitch;
				gh = in_h + (long)sub * a.h_pitch + Wd;
			} else {
				gl = in_h + (long)(Hd + sub) * a.h_pitch;
				gh = gl + Wd;
			}
			// interleaved sample i of the row, reflected into it
			auto sample = [&](int i) {
				i = refl_h(i, a.W);
				return (unsigned)((i & 1) ? gh[i >> 1] : gl[i >> 1]);
			};
			if (full) {
#pragma unroll
				for (int i = 0; i < NS; i += 2) {
					raw[rr].l[i >> 1] = load_pair(gl + cl + i);
					raw[rr].h[i >> 1] = load_pair(gh + cl + i);
				}
			} else {
#pragma unroll
				for (int i = 0; i < NS; i += 2) {
					raw[rr].l[i >> 1] = pack_bits(sample(c + 2 * i), sample(c + 2 * i + 2));
					raw[rr].h[i >> 1] = pack_bits(sample(c + 2 * i + 1), sample(c + 2 * i + 3));
				}
			}
			if (inside) {
				raw[rr].hl = load_pair(gh + cl - 2);
				raw[rr].ll = gl[cl - 1];
				raw[rr].lr = load_pair(gl + cl + NS);
				raw[rr].hr = load_pair(gh + cl + NS);
			} else {
				raw[rr].hl = pack_bits(sample(c - 3), sample(c - 1));
				raw[rr].ll = sample(c - 2);
				raw[rr].lr = pack_bits(sample(c + CPT), sample(c + CPT + 2));
				raw[rr].hr = pack_bits(sample(c + CPT + 1), sample(c + CPT + 3));
			}
		}
	};

	T st[K][1][CPT];
#pragma unroll
	for (int s = 0; s < K; s++)
#pragma unroll
		for (int v = 0; v < CPT; v++)
			st[s][0][v] = 0;

	InvRawH<CPT> q[kAheadH + 1][2]; // q[0]: this iteration's rows
#pragma unroll
	for (int d = 0; d < kAheadH; d++)
		if (d < n_iter)
			fetch(d, q[d]);
	for (int it = 0; it < n_iter; it++) {
		if (it + kAheadH < n_iter)
			fetch(it + kAheadH, q[kAheadH]);
		const InvRawH<CPT> (&cur)[2] = q[0];
		const int p = p0 + it;
		// rows first: x[j] = sample c - 3 + j of the row (x[0] odd), descaled; the K steps; the lane's columns at x[3 .. 3 + CPT - 1]
		// (both rows at once, as the halves of packed operations: the steps and the rounding of W::inv_scale / inv_step)
		T val[2][CPT];
		{
			const InvRawH<CPT> &q0 = cur[0], &q1 = cur[1];
			const float z0 = W::inv_scale(0, 1.0f), z1 = W::inv_scale(1, 1.0f); // (the descaling factors themselves)
			f2 x[NARR];
			x[0] = f2{half_of(q0.hl, 0), half_of(q1.hl, 0)} * z1;
			x[1] = f2{half_of(q0.ll, 0), half_of(q1.ll, 0)} * z0;
			x[2] = f2{half_of(q0.hl, 1), half_of(q1.hl, 1)} * z1;
#pragma unroll
			for (int i = 0; i < NS; i++) {
				x[K - 1 + 2 * i] = f2{half_of(q0.l[i >> 1], i & 1), half_of(q1.l[i >> 1], i & 1)} * z0;
				x[K + 2 * i] = f2{half_of(q0.h[i >> 1], i & 1), half_of(q1.h[i >> 1], i & 1)} * z1;
			}
			x[K - 1 + CPT] = f2{half_of(q0.lr, 0), half_of(q1.lr, 0)} * z0;
			x[K + CPT] = f2{half_of(q0.hr, 0), half_of(q1.hr, 0)} * z1;
			x[K + 1 + CPT] = f2{half_of(q0.lr, 1), half_of(q1.lr, 1)} * z0;
			x[K + 2 + CPT] = f2{half_of(q0.hr, 1), half_of(q1.hr, 1)} * z1;
#pragma unroll
			for (int s = 0; s < K; s++) {
#pragma unroll
				for (int j = s + 1; j <= NARR - 2 - s; j += 2)
					x[j] = x[j] + W::ik(s) * (x[j - 1] + x[j + 1]);
			}
#pragma unroll
			for (int v = 0; v < CPT; v++) {
				const f2 sc = x[K - 1 + v] * f2{z0, z1}; // (the vertical pass descales by ROW parity)
				val[0][v] = sc[0];
				val[1][v] = sc[1];
			}
		}
		// then the columns: the rows 2p - 3 and 2p - 2 are final
		T odd_row[CPT], even_row[CPT];
		inv_vertical<W, kColNone>(val[0], val[1], st, 0, odd_row, even_row);
		const int pe = p - 1, po = p - 2;
		const bool ve = pe >= A && pe < B;
		const bool vo = po >= A && po < B && (2 * po + 1 < a.H);
		const int n = a.W - c;
		// the level's only rounding
		if (vo) {
			unsigned v[CPT / 2];
#pragma unroll
			for (int i = 0; i < CPT / 2; i++)
				v[i] = pack_pair(odd_row[2 * i], odd_row[2 * i + 1]);
			hbits *d = out + (long)(2 * po + 1) * a.out_pitch + c;
			if (a.temporal_out)
				store_samples<false>(d, v, n);
			else
				store_samples<true>(d, v, n);
		}
		if (ve) {
			unsigned v[CPT / 2];
#pragma unroll
			for (int i = 0; i < CPT / 2; i++)
				v[i] = pack_pair(even_row[2 * i], even_row[2 * i + 1]);
			hbits *d = out + (long)(2 * pe) * a.out_pitch + c;
			if (a.temporal_out)
				store_samples<false>(d, v, n);
			else
				store_samples<true>(d, v, n);
		}
#pragma unroll
		for (int d = 0; d < kAheadH; d++) {
			q[d][0] = q[d + 1][0];
			q[d][1] = q[d + 1][1];
		}
	}
}

hipError_t launch_inv_level_h(Wavelet w, const InvLevelArgs &a, const SweepTuning &t, hipStream_t s)
{
	if (w != kCdf97H || a.W < 2 || a.H < 2 || a.batch < 1 || a.interleaved)
		return hipErrorInvalidValue;
	constexpr int TW = 64 * kInvCptH;
	SweepGeom g;
	const int Hd = (a.H + 1) / 2;
	g.ntx = (a.W + TW - 1) / TW;
	g.tile_pairs = h_tile_pairs(t, g.ntx, Hd, (long)a.W * a.H * a.batch, a.batch, 32, 2048);
	g.swz = t.xcd_swizzle;
	g.wave_horiz = 0;
	const int waves = sweep_waves(t);
	const dim3 grid = sweep_grid(g, (Hd + g.tile_pairs - 1) / g.tile_pairs, waves, a.batch);
	k_inv_sweep_h<Cdf97H, kInvCptH><<<grid, 64 * waves, 0, s>>>(a, g);
	return hipGetLastError();
}

// ---- the line-pass route: a frame of binary16 samples <-> a frame of binary32 -------------------------------------------
// The exact line passes of a level run Cdf97S on a binary32 copy of its frame, so that the row pass's result is not rounded
// to binary16 before the column pass reads it: k_frame_cvt widens the frame before the passes and narrows it after them.
// w x h samples, rows `hp` / `fp` bytes apart; any 2-byte alignment of the binary16 side.
template <bool WIDEN>
__global__ __launch_bounds__(256) void k_frame_cvt(char *halves, long hp, char *floats, long fp, int w, int h)
{
	const int x = blockIdx.x * blockDim.x + threadIdx.x;
	if (x >= w)
		return;
	for (int y = blockIdx.y; y < h; y += gridDim.y) {
		hbits *ph = (hbits *)(halves + (long)y * hp) + x;
		float *pf = (float *)(floats + (long)y * fp) + x;
		if constexpr (WIDEN)
			*pf = widen(*ph);
		else
			*ph = (hbits)narrow(*pf);
	}
}

hipError_t launch_half_frame_cvt(bool widen_, void *halves, long half_pitch, void *floats, long float_pitch, int w, int h, hipStream_t s)
{
	if (w <= 0 || h <= 0)
		return hipSuccess;
	const dim3 grid((w + 255) / 256, h < 65535 ? h : 65535);
	if (widen_)
		k_frame_cvt<true><<<grid, 256, 0, s>>>((char *)halves, half_pitch, (char *)floats, float_pitch, w, h);
	else
		k_frame_cvt<false><<<grid, 256, 0, s>>>((char *)halves, half_pitch, (char *)floats, float_pitch, w, h);
	return hipGetLastError();
}

} // namespace dwt
