// dwt_backend.hip -- device context, workspace, host<->HBM staging and the multi-level
// drivers behind the C-ABI of include/libdwt_hip.h.
//
// Level scheduling (forward, dense frame).  libdwt transforms in place
// (src/libdwt.c:12812-12919): level j reads the LL region of the image and writes
// its four subbands over it.  A fused tile sweep cannot do that (one tile's outputs
// land on another tile's inputs), so the driver keeps the running LL band in a
// small ping-pong scratch instead of the image:
//
//     level 0 : image            -> HL/LH/HH at their final place, LL -> scratch0
//     level j : scratch[(j-1)&1] -> HL/LH/HH at their final place, LL -> scratch[j&1]
//     last    :                     LL -> its final place too
//   (large out-of-place float 9/7 calls: levels 0 and 1 in one launch, image -> both levels' HL/LH/HH, LL -> scratch1;
//    pair01_ok below -- and levels 2 and 3, 4 and 5 ... of those calls likewise, scratch to scratch: pair_deep_ok)
//
// Every level therefore reads its input once and writes its output once: the
// algorithmic traffic 2*sizeof(T)*sum_j(W_j*H_j).  Only when the caller's source
// and destination are the SAME device buffer does level 0 have to detour its detail
// subbands through a staging image and copy them back (the `_s2` entries and every
// host-pointer call avoid that).  The inverse runs the mirror image of this.
//
// Frames with size_o != size_i, zero padding, and levels where a direction has a
// single line follow the reference's exact line-by-line semantics through the
// generic line-pass kernel, out of place per pass (generic_level).
//
// Which of the two a level takes is a function of the call alone: its entry builds a Call2d (call2d) from the wavelet and
// the images the transform runs on, and the drivers, level_fused_ok and the tuners take that value as an argument.
#include "dwt_backend.h"

namespace dwtb {

thread_local Ctx g;
thread_local char g_err[512] = "";

int fail(const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof(g_err), fmt, ap);
	va_end(ap);
	return 1;
}

int launched(hipError_t e, const char *family, const char *what)
{
	g.stat_launches++;
	return e == hipSuccess ? 0 : fail("%s %s launch failed: %s", family, what, hipGetErrorString(e));
}

static bool dword_aligned(std::initializer_list<const void *> ptrs, std::initializer_list<long> strides)
{
	bool ok = true;
	for (const void *p : ptrs)
		ok = ok && (uintptr_t)p % 4 == 0;
	for (long s : strides)
		ok = ok && s % 4 == 0;
	return ok;
}

int check_dev_align(std::initializer_list<const void *> ptrs, std::initializer_list<long> strides)
{
	return dword_aligned(ptrs, strides) ? 0 : fail("device memory takes strides and addresses that are multiples of 4 bytes");
}

Call2d call2d(Wavelet w, std::initializer_list<const void *> ptrs, std::initializer_list<long> strides)
{
	return Call2d{w, elem_size(w), dword_aligned(ptrs, strides)};
}

int grow(Buf &b, size_t need)
{
	if (b.bytes >= need)
		return 0;
	if (b.p) {
		HIP_TRY(hipStreamSynchronize(g.stream));
		drop(b);
	}
	HIP_TRY(hipMalloc(&b.p, need));
	g.stat_allocs++;
	b.bytes = need;
	return 0;
}

void drop(Buf &b)
{
	if (b.p)
		dev_free(b.p);
	b = Buf{};
}

// several rectangles (element coordinates) between two device images in one kernel launch
struct Rect {
	long dx, dy, sx, sy, w, h;
};
static CopyRects make_copy_rects(Img dst, Img src, const Rect *rc, int n, int policy)
{
	CopyRects r{};
	r.n = 0;
	r.policy = policy;
	for (int k = 0; k < n && r.n < 3; k++) {
		if (rc[k].w <= 0 || rc[k].h <= 0)
			continue;
		const int i = r.n++;
		r.src[i] = src.p + rc[k].sy * src.sx + rc[k].sx * src.es;
		r.dst[i] = dst.p + rc[k].dy * dst.sx + rc[k].dx * dst.es;
		r.spitch[i] = src.sx;
		r.dpitch[i] = dst.sx;
		r.wbytes[i] = (int)(rc[k].w * dst.es);
		r.h[i] = (int)rc[k].h;
	}
	return r;
}

// the staged subbands of an in-place call between the image and the staging image: one launch of the rectangle kernel --
// which moves whole dwords, so 2-byte elements go by plain 2-D copies
static int copy_staged(Img dst, Img src, const Rect *rc, int n, int policy)
{
	if (dst.es != 2)
		return launched(launch_copy_rects(make_copy_rects(dst, src, rc, n, policy), g.stream), "rectangle", "copy");
	for (int k = 0; k < n; k++)
		if (copy_rect(dst, rc[k].dx, rc[k].dy, src, rc[k].sx, rc[k].sy, rc[k].w, rc[k].h))
			return 1;
	return 0;
}

// A rectangle copy that RIDES ALONG with the levels it does not depend on (one image, in place: the staged subbands of
// level 0 going back / aside): its blocks are handed out to those levels' launches as extra workgroups behind their
// tiles (FwdLevelArgs::ride).  The levels below level 0 of one image are latency-bound -- one round of waves, 9-33 us
// each, the memory system mostly idle -- and the copy is bandwidth-bound (402 MB, 62 us as a launch of its own): together
// they take what the larger of the two takes.  Whatever is left when the levels are through goes out as a plain launch.
struct RideCopy {
	CopyRects r;
	int next = 0, total = 0;
	bool on = false;
	// blocks for a level with `own_bytes` of input when `carriers_after` later launches can take some too
	int share(size_t own_bytes, int carriers_after) const
	{
		const int left = total - next;
		const int small = std::min(left, g.ride_mib * 32); // blocks of 32 KiB
		if (carriers_after <= 0)
			return left;
		if (own_bytes <= ((size_t)32 << 20))
			return small;
		return std::max(small, left - carriers_after * g.ride_mib * 32);
	}
	int flush()
	{
		if (!on || next >= total)
			return 0;
		const int from = next;
		next = total;
		return launched(launch_copy_rects_range(r, from, total, g.stream), "rectangle", "copy");
	}
};

int copy_rect_on(hipStream_t st, Img dst, long dx, long dy, Img src, long sx_, long sy_, long w, long h)
{
	if (w <= 0 || h <= 0)
		return 0;
	HIP_TRY(hipMemcpy2DAsync(dst.p + dy * dst.sx + dx * dst.es, dst.sx, src.p + sy_ * src.sx + sx_ * src.es, src.sx, w * dst.es, h,
		hipMemcpyDeviceToDevice, st));
	return 0;
}
int copy_rect(Img dst, long dx, long dy, Img src, long sx_, long sy_, long w, long h)
{
	return copy_rect_on(g.stream, dst, dx, dy, src, sx_, sy_, w, h);
}

int zero_rect(Img img, long x, long y, long w, long h)
{
	if (w <= 0 || h <= 0)
		return 0;
	HIP_TRY(hipMemset2DAsync(img.p + y * img.sx + x * img.es, img.sx, 0, w * img.es, h, g.stream));
	return 0;
}

// One generic 1-D pass over the frame of a level (rows: lines are image rows).
// in == out is handled by staging the frame -- pass-through elements included -- in
// an image with the caller's pitch, so the kernel sees one pair of strides.
int generic_pass(Wavelet w, bool inverse, bool rows, Img in, Img out, int frame_w, int frame_h, int n_lines, int N, int hoff)
{
	if (n_lines <= 0 || N <= 0)
		return 0;
	if (N == 1 && facts(w).lone) {
		// the int kernels leave a lone sample as it is (src/libdwt.c:10961); out of place that
		// still means the samples have to arrive in the destination
		if (in.p != out.p)
			return copy_rect(out, 0, 0, in, 0, 0, frame_w, frame_h);
		return 0;
	}
	const bool alias = in.p == out.p;
	Img dst = out;
	if (alias) {
		// staging image with the SAME pitch as the caller's image
		if (grow(g.stage_img, (size_t)out.sx * frame_h))
			return 1;
		dst = Img{(char *)g.stage_img.p, out.sx, out.es};
		if (copy_rect(dst, 0, 0, out, 0, 0, frame_w, frame_h))
			return 1;
	} else if (in.sx != out.sx) {
		return fail("generic pass: source and destination pitches differ (%ld vs %ld)", in.sx, out.sx);
	}
	if (launched(launch_line_pass(w, inverse, in.p, dst.p, rows ? in.sx : in.es, rows ? in.es : in.sx, n_lines, N, hoff, !rows, g.stream), "line", "pass"))
		return 1;
	if (alias && copy_rect(out, 0, 0, dst, 0, 0, frame_w, frame_h))
		return 1;
	return 0;
}

void prof_before(int level)
{
	g.stat_launches++; // (every fused level launch of the 2-D drivers passes here)
	if (!g.prof_on || (g.prof_on == 1 && level != 0))
		return;
	if (g.prof_tag.size() <= g.prof_used)
		g.prof_tag.resize(g.prof_used + 1);
	g.prof_tag[g.prof_used] = level;
	if (g.prof_used == g.prof_events.size()) {
		hipEvent_t a, b;
		hipEventCreate(&a);
		hipEventCreate(&b);
		g.prof_events.push_back({a, b});
	}
	hipEventRecord(g.prof_events[g.prof_used].first, g.stream);
}

void prof_after(int level)
{
	if (!g.prof_on || (g.prof_on == 1 && level != 0))
		return;
	hipEventRecord(g.prof_events[g.prof_used].second, g.stream);
	g.prof_used++;
}

int prof_drain()
{
	if (g.prof_used == 0)
		return 0;
	HIP_TRY(hipStreamSynchronize(g.stream));
	for (size_t i = 0; i < g.prof_used; i++) {
		float ms = 0;
		HIP_TRY(hipEventElapsedTime(&ms, g.prof_events[i].first, g.prof_events[i].second));
		const int lv = g.prof_tag[i] & 15;
		g.prof_level_ms[lv] += ms;
		g.prof_level_n[lv]++;
		if (lv == 0) {
			g.prof_ms += ms;
			g.prof_launches++;
		}
	}
	g.prof_used = 0;
	return 0;
}

long ll_pitch_elems(int w) { return align_up(w, 4); }
static char *ll_band(int k) { return (char *)g.ll[k].p; }

size_t ll_band_bytes(const Geom &ge, int k, int batch, int es)
{
	return (size_t)ll_pitch_elems(ge.Wo(k + 1)) * ge.Ho(k + 1) * es * batch + 64;
}

int ensure_ll(const Geom &ge, int batch, int es)
{
	for (int k = 0; k < 2; k++) {
		if (g.ll_external) {
			if (g.ll[k].bytes < ll_band_bytes(ge, k, batch, es))
				return fail("the caller's workspace (dwt_hip_set_workspace) is too small: band %d needs %zu bytes", k, ll_band_bytes(ge, k, batch, es));
			continue;
		}
		if (grow(g.ll[k], ll_band_bytes(ge, k, batch, es)))
			return 1;
	}
	return 0;
}

// the fused sweeps exist for the 32-bit types and, since round 2, for the double-precision wavelets
// (dwt_sweep2d_d.hip; option "fused_d" = 0 sends those back to the exact line passes); the int16 5/3 and the float 9/7 on
// binary16 storage have their own (dwt_sweep2d_i16.hip, dwt_sweep2d_h.hip) for the calls whose images call2d found aligned
bool level_fused_ok(const Call2d &c, const Geom &ge, int j)
{
	return !g.force_generic && (c.es == 4 || (c.es == 2 ? c.aligned : g.fused_d != 0)) && ge.Wi(j) == ge.Wo(j) && ge.Hi(j) == ge.Ho(j) && ge.Wo(j) >= 2 &&
		ge.Ho(j) >= 2;
}
// Levels 0 and 1 of a forward transform in ONE launch (launch_fwd01: the level-0 sweep's own 512-column tiles, level 0's LL
// band never written): float 9/7 without contraction, Mallat layout, out of place (no staging detour, no copy riding along),
// two levels or more, both fused, W and H multiples of 4 with both levels of 64 x 64 or more, and none of the sweep's
// geometry set by hand to something the fused kernel is not (its tiles are the 8-column ones of the deep-ring level sweep; the
// depth of its OWN ring -- 16 rows, or 8 for two workgroups per CU -- is option fuse01_ring, the tuner's choice or the rule
// above launch_fwd01, never `ring`).  Option fuse01: 0 never, 2 wherever that holds, 1 (default) where it also pays:
//   - the launch costs about level 0 x 1.05 (level 1's warm-up rows) x 1.03 (its arithmetic, stores and phantom columns)
//     against level 0 + level 1 = 1.25 x level 0, whatever the width: the tiles are level 0's, so no width is kept out;
//   - only in launches of 32768 tiles of 512 columns x 64 pairs and more (32 images of 8192^2), the sizes it was measured
//     to win at (profiles/fuse01_summary.md, profiles/fuse01_seams_summary.md).  Below 3072 tiles level 0 does not take
//     the deep ring itself -- a round or two of waves wants the shallow ring's 8 waves per CU --; in between nothing was
//     measured, and a call on 16 images of 8192^2 is held to one launch per level (tests/test_hip_multi.py).
//
// The same launch takes levels (j, j + 1) at any even j: the kernel reads `in` and addresses both levels' detail quadrants
// from the image's top left corner, and nothing in it knows its level.  A deeper pair reads the running band from one scratch
// band and leaves level j + 1's in the other (or in the image when it is the last), greedy from the top: (0, 1), (2, 3),
// (4, 5) ...; a level left over runs alone.  What a pair at j needs is what the pair at 0 needs, of level j: pair_legal.
// Option fuse_deep for j >= 2: 0 never, 2 wherever legal, 1 (default) where it was measured to pay
// (profiles/fuse_deep_summary.md): only in a call whose levels 0 and 1 engaged by their size rule -- so 16 images of 8192^2,
// every single image and every small call stay at one launch per level --, and only in launches of kDeepTiles tiles of 512
// columns x 64 pairs and more, the smallest launch the measurement covers and a winner already: levels 2 + 3 against the pair,
// the whole 5-level call tuned by dwt_hip_tune, one process, alternated, placed buffers: 64 x 8192^2 (4096 tiles) 534 -> 381 us,
// 256 x 4096^2 (4096 tiles) 478 -> 367 us, 32 x 8192^2 (2048 tiles) 277 -> 223 us, the spread of the two launches 5 us.
static long pair_tiles(const Geom &ge, int j, int batch)
{
	return (long)fwd01_tiles(ge.Wo(j)) * (((ge.Ho(j) >> 1) + 63) / 64) * batch;
}

static bool pair_legal(const Call2d &c, const Geom &ge, int J, int j)
{
	if ((j & 1) || g.fma || j + 1 >= J || !level_fused_ok(c, ge, j) || !level_fused_ok(c, ge, j + 1) || !fwd01_can(c.w, ge.Wo(j), ge.Ho(j)))
		return false;
	const SweepTuning &t = g.tune;
	return !(t.cpt == 4 || t.ring == 8 || (t.nt & 8) || (t.tile_pairs & 1));
}

// levels 0 and 1; *by_size: the pair engages by the size rule (whatever fuse01 = 2 adds)
static bool pair01_ok(const Call2d &c, const Geom &ge, int J, int batch, bool *by_size)
{
	*by_size = g.fuse01 && pair_legal(c, ge, J, 0) && pair_tiles(ge, 0, batch) >= 32768;
	return *by_size || (g.fuse01 >= 2 && pair_legal(c, ge, J, 0));
}

// levels (j, j + 1), j >= 2; pair01_by_size: this call's levels 0 and 1 ran as a pair, by the size rule
constexpr long kDeepTiles = 2048;
// The ring rows, the direction and the tile height of a deeper pair's launch of kDeepTiles tiles and more, where they are
// neither set by hand nor measured by dwt_hip_tune (below that size: the launcher's rule for small launches, as for the pair
// at 0): the 8-row ring, odd tile rows upward, 128 row pairs where that leaves two tile rows or more.  Rings 8 / 16 x every
// row downward / odd rows upward x 32 / 64 / 128 pairs on the three launches above, untuned: this one is first on the two of
// 4096 tiles -- 128 pairs make them ONE round of the 2048 resident waves -- (381 and 367 us; at 64 pairs 428 and 407, the 16-row
// ring at its best 417 and 413, every row downward 430 and 372) and within 7 % of the first on 32 x 8192^2 (224 us against 209
// for the 16-row ring at 128 pairs: half a round either way).  The launcher's rule for this size (16 rows, downward, 64 pairs):
// 518, 475 and 270 us.  profiles/fuse_deep_summary.md.
constexpr int kDeepRing = 8, kDeepUpDown = 1, kDeepPairs = 128;
static bool pair_deep_ok(const Call2d &c, const Geom &ge, int J, int batch, int j, bool pair01_by_size)
{
	if (!g.fuse_deep || j < 2 || !pair_legal(c, ge, J, j))
		return false;
	return g.fuse_deep >= 2 || (pair01_by_size && pair_tiles(ge, j, batch) >= kDeepTiles);
}

// ---- the line-pass route of the float 9/7 on binary16 storage (kCdf97H) ----------------
// A level rounds ONCE: its exact line passes are those of the float 9/7 (kCdf97S) on binary32 copies of the level's frame,
// widened before the passes (exact) and narrowed after them (round to nearest even).  half_level_begin: the Wo x Ho frame of
// `cur` -- and that of `dst` where it is another image: the passes leave the elements they do not write as the destination
// has them -- in binary32 (Ctx::half_f32); half_level_end: the destination's copy narrowed into dst.  Elements no pass writes
// go through both conversions and keep their value, except the payload of a signalling NaN, which the widening quiets.
static int half_level_begin(Img cur, Img dst, int Wo, int Ho, Img *fcur, Img *fdst)
{
	const long fp = align_up((long)Wo * 4, 256);
	if (grow(g.half_f32, (size_t)fp * Ho * 2))
		return 1;
	*fcur = Img{(char *)g.half_f32.p, fp, 4};
	if (launched(launch_half_frame_cvt(true, cur.p, cur.sx, fcur->p, fp, Wo, Ho, g.stream), "binary16 frame", "widening"))
		return 1;
	*fdst = *fcur;
	if (cur.p != dst.p) {
		*fdst = Img{(char *)g.half_f32.p + (size_t)fp * Ho, fp, 4};
		if (launched(launch_half_frame_cvt(true, dst.p, dst.sx, fdst->p, fp, Wo, Ho, g.stream), "binary16 frame", "widening"))
			return 1;
	}
	return 0;
}

static int half_level_end(Img fdst, Img dst, int Wo, int Ho)
{
	return launched(launch_half_frame_cvt(false, dst.p, dst.sx, fdst.p, fdst.sx, Wo, Ho, g.stream), "binary16 frame", "narrowing");
}

// ---- one level on the exact line passes, both directions ---------------------------------
// The Wo x Ho frame of `in` -> that of `out` (forward: the running image and dst; inverse: dst and dst); Wi x Hi: the
// frame's inner sizes, (Wh, Hh): where the H halves start.  The passes run as the call's wavelet on its own images, or
// (binary16 storage) as the float 9/7 on binary32 copies of the frame.  Zero padding stays with the drivers.
static int generic_level(const Call2d &c, bool inverse, Img in, Img out, int Wo, int Ho, int Wi, int Hi, int Wh, int Hh)
{
	const WaveletFacts &f = facts(c.w);
	const bool cols_first = inverse ? f.cols_inv : f.cols_fwd;
	Img lc = in, ld = out;
	if (widened(c.w) && half_level_begin(in, out, Wo, Ho, &lc, &ld))
		return 1;
	// dense frame: each pass writes every element of the level's frame, so the two passes
	// ping-pong through the staging image (first pass: image -> stage, second: stage -> image)
	// instead of each staging and copying back a frame of its own: 4 instead of 12 frame
	// transfers per level (the double-precision drivers and accel 1 live on these passes)
	const bool dense = Wi == Wo && Hi == Ho && Wo >= 2 && Ho >= 2;
	if (dense && grow(g.stage_img, (size_t)ld.sx * Ho))
		return 1;
	for (int pass = 0; pass < 2; pass++) {
		const bool rows = cols_first != (pass == 0);
		if (f.skip1 && (rows ? Wo : Ho) <= 1)
			continue;
		const Img to = dense && pass == 0 ? Img{(char *)g.stage_img.p, ld.sx, ld.es} : ld;
		if (generic_pass(f.line_as, inverse, rows, lc, to, Wo, Ho, rows ? Ho : Wo, rows ? Wi : Hi, rows ? Wh : Hh))
			return 1;
		lc = to; // the second pass reads what the first wrote -- the input itself where that one was skipped (src/libdwt.c:12709, :12742)
	}
	return widened(c.w) ? half_level_end(ld, out, Wo, Ho) : 0;
}

// ---- one fused level: the sweep of the call's element type -------------------------------
static hipError_t sweep_fwd(const Call2d &c, const FwdLevelArgs &a, const SweepTuning &t, hipStream_t s)
{
	return c.es == 8 ? launch_fwd_level_d(c.w, a, t, s)
	     : c.es == 4 ? launch_fwd_level(sweep32_wavelet(c.w), a, t, s)
	     : widened(c.w) ? launch_fwd_level_h(c.w, a, t, s) // (2-byte elements: binary16 storage, or the int16 5/3)
	                    : launch_fwd_level_i16(c.w, a, t, s);
}

static hipError_t sweep_inv(const Call2d &c, const InvLevelArgs &a, const SweepTuning &t, hipStream_t s)
{
	return c.es == 8 ? launch_inv_level_d(c.w, a, t, s)
	     : c.es == 4 ? launch_inv_level(sweep32_wavelet(c.w), a, t, s)
	     : widened(c.w) ? launch_inv_level_h(c.w, a, t, s)
	                    : launch_inv_level_i16(c.w, a, t, s);
}

// ---- forward ---------------------------------------------------------------------
int forward2d(const Call2d &c, Img src, Img dst, const Geom &ge, int *jp, int decompose_one, int zero_padding,
	int batch, long src_bstride, long dst_bstride)
{
	const int so_min = ge.sox < ge.soy ? ge.sox : ge.soy, so_max = ge.sox > ge.soy ? ge.sox : ge.soy;
	const int j_limit = ceil_log2(decompose_one ? so_max : so_min);
	if (*jp < 0 || *jp > j_limit)
		*jp = j_limit; // src/libdwt.c:12807-12810
	const int J = *jp;
	if (J == 0)
		return 0;
	const Wavelet w = c.w;
	const int es = c.es;
	if (ensure_ll(ge, batch, es))
		return 1;

	// where the running LL band lives: -1 = in `cur` image (src before level 0, dst after), else scratch index
	int ll_in = -1;
	Img cur = src;
	RideCopy ride;
	bool pair01_by_size = false; // levels 0 and 1 ran as a pair by the size rule: what the deeper pairs' own rule asks first
	g.stat_deep_pairs = 0;
	// the fused levels from j on that can carry copy blocks (one image, a sweep variant with the ride-along kernel)
	auto carriers_from = [&](int j0) {
		int n = 0;
		for (int j = j0; j < J && level_fused_ok(c, ge, j); j++)
			n += es == 4 && sweep_ride_ok(g.tune, ge.Wo(j), ge.Ho(j), batch, false);
		return n;
	};
	for (int j = 0; j < J; j++) {
		const int Wo = ge.Wo(j), Ho = ge.Ho(j), Wi = ge.Wi(j), Hi = ge.Hi(j);
		const int Wd = ge.Wo(j + 1), Hd = ge.Ho(j + 1);
		if (level_fused_ok(c, ge, j)) {
			// (a fused pair: levels 0 and 1 of an out-of-place call, or levels (j, j + 1) from scratch while no copy waits for a
			// launch to ride along with; jl: the level whose LL band leaves the launch)
			bool by_size = false;
			const bool pair = j == 0 ? ll_in < 0 && cur.p != dst.p && pair01_ok(c, ge, J, batch, &by_size)
			                         : ll_in >= 0 && !(ride.on && ride.next < ride.total) && pair_deep_ok(c, ge, J, batch, j, pair01_by_size);
			if (j == 0)
				pair01_by_size = pair && by_size;
			else if (pair)
				g.stat_deep_pairs++;
			const int jl = pair ? j + 1 : j;
			const bool last = (jl == J - 1) || !level_fused_ok(c, ge, jl + 1);
			FwdLevelArgs a;
			a.W = Wo;
			a.H = Ho;
			a.batch = batch;
			bool detour = false;
			if (ll_in < 0) {
				a.in = cur.p;
				a.in_pitch = cur.sx / es;
				a.in_bstride = (cur.p == src.p ? src_bstride : dst_bstride) / es;
				detour = (cur.p == dst.p); // reading the image we also write: stage the outputs
			} else {
				a.in = ll_band(ll_in);
				a.in_pitch = ll_pitch_elems(Wo);
				a.in_bstride = a.in_pitch * Ho;
			}
			Img hdst = dst;
			long h_bstride = dst_bstride;
			if (detour) {
				if (batch != 1)
					return fail("in-place batches are not supported; use distinct src and dst");
				if (grow(g.stage_img, (size_t)dst.sx * Ho))
					return 1;
				hdst = Img{(char *)g.stage_img.p, dst.sx, es};
				h_bstride = 0;
				// a copy-back that follows at once reads the staged subbands out of the 256 MiB Infinity Cache when they were
				// stored temporal (one 8192^2 image: 218.5 -> 205 us); a copy that rides along with the deeper levels is spread
				// over their launches and gains nothing from it (202 against 205 us)
				a.temporal = (g.ride_copy && carriers_from(j + 1) > 0) ? 0 : 1;
			}
			a.out_h = hdst.p;
			a.h_pitch = hdst.sx / es;
			a.h_bstride = h_bstride / es;
			// ping-pong: the other buffer than the one read; band j+1 fits either for j >= 1.  A fused pair writes level 1's
			// band where the two launches would have left it, in scratch 1 (scratch 0 is sized for level 0's band, unused then);
			// a deeper pair reads one scratch band and writes the other, which holds any band below level 1's
			const int ll_out = last ? -1 : (ll_in < 0 ? (jl & 1) : 1 - ll_in);
			if (last) {
				a.out_ll = hdst.p;
				a.ll_pitch = a.h_pitch;
				a.ll_bstride = a.h_bstride;
			} else {
				a.out_ll = ll_band(ll_out);
				a.ll_pitch = ll_pitch_elems(ge.Wo(jl + 1));
				a.ll_bstride = a.ll_pitch * ge.Ho(jl + 1);
			}
			SweepTuning tune = g.tune;
			if (pair && j == 0)
				g.stat_choice01 = 0;
			// (a deeper pair of the size its rule engages it at: ring, direction and height by that rule (kDeepRing ...) unless set
			// by hand or measured -- the launcher's rule for launches of this size is that of the small forced pairs)
			const bool deep_rule = pair && j > 0 && pair_tiles(ge, j, batch) >= kDeepTiles;
			if (deep_rule && !tune.fuse01_ring)
				tune.fuse01_ring = kDeepRing;
			if (es == 4 && tune.tile_pairs <= 0) {
				const int choice = pair ? tuned_tile_pairs01(w, a) : tuned_tile_pairs(w, a); // (0, nothing measured: the launcher's own rule)
				apply_tile_choice(choice, &tune, pair ? kTileFwd01 : kTileFwd);
				if (pair && j == 0)
					g.stat_choice01 = choice;
				if (deep_rule && choice <= 0 && (Ho >> 1) >= 2 * kDeepPairs)
					tune.tile_pairs = kDeepPairs;
			}
			if (pair) {
				// the direction of the tile rows: the option, else what dwt_hip_tune measured at this height and depth, else the rule
				const int dir = tuned_updown01(w, a, tune);
				if (dir >= 0)
					tune.fuse01_updown = dir;
				else if (deep_rule && tune.fuse01_updown < 0)
					tune.fuse01_updown = kDeepUpDown;
				if (j == 0)
					g.stat_updown01 = fwd01_updown(tune, a.W, a.H, a.batch);
			}
			if (ride.on && ride.next < ride.total && es == 4 && sweep_ride_ok(tune, Wo, Ho, batch, false)) {
				a.ride = &ride.r;
				a.ride_lo = ride.next;
				a.ride_hi = ride.next + ride.share((size_t)Wo * Ho * es, carriers_from(j + 1));
				ride.next = a.ride_hi;
			}
			prof_before(j);
			hipError_t e = pair ? launch_fwd01(a, tune, g.stream) : sweep_fwd(c, a, tune, g.stream);
			prof_after(j);
			if (e != hipSuccess)
				return fail("forward level %d launch failed: %s", j, hipGetErrorString(e));
			if (detour) {
				// copy the staged subbands to their place: right half, bottom-left, and the LL
				// quadrant too when it was written here (in line: on a side stream beside the deeper
				// levels it measured 8-10 us slower, profiles/archive/r03_entries_summary.md)
				const Rect rc[3] = {{Wd, 0, Wd, 0, Wo - Wd, Ho}, {0, Hd, 0, Hd, Wd, Ho - Hd}, {0, 0, 0, 0, last ? Wd : 0, Hd}};
				if (es == 4) {
					ride.r = make_copy_rects(dst, hdst, rc, 3, 3);
					ride.total = copy_rects_plan(&ride.r);
					ride.next = 0;
					ride.on = g.ride_copy && ride.total > 0 && carriers_from(j + 1) > 0;
				}
				if (!ride.on && copy_staged(dst, hdst, rc, 3, 3))
					return 1;
			}
			ll_in = ll_out;
			cur = dst;
			j = jl;
			continue;
		}

		// ---- generic level: exact line semantics, in place on dst ----
		if (ride.flush()) // (the line passes borrow the staging image the copy still reads)
			return 1;
		if (batch != 1)
			return fail("batched transforms need dense frames with both sides >= 2 at every level");
		if (ll_in >= 0) {
			// bring the LL band back into the image
			Img s{ll_band(ll_in), ll_pitch_elems(Wo) * es, es};
			if (copy_rect(dst, 0, 0, s, 0, 0, Wo, Ho))
				return 1;
			ll_in = -1;
			cur = dst;
		}
		if (generic_level(c, false, cur, dst, Wo, Ho, Wi, Hi, Wd, Hd))
			return 1;
		cur = dst; // (a pass ran: a level has a side of 2 or more, and only a direction of ONE line is ever skipped)
		if (zero_padding) {
			// dwt_zero_padding_f_stride_* (src/libdwt.c:12079-12131) over rows then columns
			const int nl_x = (Wi + 1) >> 1, nh_x = Wi >> 1, nl_y = (Hi + 1) >> 1, nh_y = Hi >> 1;
			if (zero_rect(dst, nl_x, 0, Wd - nl_x, Ho) || zero_rect(dst, Wd + nh_x, 0, (Wo - Wd) - nh_x, Ho) ||
				zero_rect(dst, 0, nl_y, Wo, Hd - nl_y) || zero_rect(dst, 0, Hd + nh_y, Wo, (Ho - Hd) - nh_y))
				return 1;
		}
	}
	return ride.flush();
}

// ---- inverse ---------------------------------------------------------------------
int inverse2d(const Call2d &c, Img src, Img dst, const Geom &ge, int j_max, int decompose_one, int zero_padding,
	int batch, long src_bstride, long dst_bstride)
{
	const int so_min = ge.sox < ge.soy ? ge.sox : ge.soy, so_max = ge.sox > ge.soy ? ge.sox : ge.soy;
	int J = ceil_log2(decompose_one ? so_max : so_min);
	if (j_max >= 0 && j_max < J)
		J = j_max; // src/libdwt.c:17069-17072
	if (J == 0) {
		// dwt_cdf97_2i_s2 still copies the inner region (src/libdwt.c:18001-18008)
		if (src.p != dst.p && copy_rect(dst, 0, 0, src, 0, 0, ge.six, ge.siy))
			return 1;
		return 0;
	}
	const Wavelet w = c.w;
	const int es = c.es;
	if (ensure_ll(ge, batch, es))
		return 1;

	// reconstruction level j consumes the subbands of size ceil(.,j) and produces the
	// band of size ceil(.,j-1); it is fused when that PRODUCED frame is dense and >= 2
	auto fused_ok = [&](int j) { return level_fused_ok(c, ge, j - 1); };

	Img cur = src;          // image holding the not-yet-consumed subbands
	long cur_bstride = src_bstride;
	int ll_in = -1;         // -1: LL band is in `cur`; else scratch index
	bool copied = false;
	// In place (one image), every level fused: the final level would overwrite subbands it still reads, so they are
	// moved aside first -- a copy that depends on none of the deeper levels and rides along with them (RideCopy)
	RideCopy ride;
	if (src.p == dst.p && batch == 1 && J >= 2 && g.ride_copy && es == 4) {
		bool all = true;
		int carriers = 0;
		for (int j = J; j >= 1; j--)
			all = all && fused_ok(j);
		for (int j = J; j >= 2; j--)
			carriers += sweep_ride_ok(g.tune, ge.Wo(j - 1), ge.Ho(j - 1), batch, true);
		if (all && carriers > 0) {
			const int Ws = ge.Wo(1), Hs = ge.Ho(1), Wo = ge.Wo(0), Ho = ge.Ho(0);
			if (grow(g.stage_img, (size_t)dst.sx * Ho))
				return 1;
			Img st{(char *)g.stage_img.p, dst.sx, es};
			const Rect rc[2] = {{Ws, 0, Ws, 0, Wo - Ws, Ho}, {0, Hs, 0, Hs, Ws, Ho - Hs}};
			ride.r = make_copy_rects(st, src, rc, 2, /* temporal both ways: the final level reads the staged subbands */ 0);
			ride.total = copy_rects_plan(&ride.r);
			ride.on = ride.total > 0;
		}
	}
	for (int j = J; j >= 1; j--) {
		const int Ws = ge.Wo(j), Hs = ge.Ho(j);       // subband sizes (= Mallat offsets)
		const int Wo = ge.Wo(j - 1), Ho = ge.Ho(j - 1); // produced frame
		const int Wi = ge.Wi(j - 1), Hi = ge.Hi(j - 1);
		if (fused_ok(j)) {
			InvLevelArgs a;
			a.W = Wo;
			a.H = Ho;
			a.batch = batch;
			a.in_h = cur.p;
			a.h_pitch = cur.sx / es;
			a.h_bstride = cur_bstride / es;
			if (ll_in < 0) {
				a.in_ll = cur.p;
				a.ll_pitch = cur.sx / es;
				a.ll_bstride = cur_bstride / es;
			} else {
				a.in_ll = ll_band(ll_in);
				a.ll_pitch = ll_pitch_elems(Ws);
				a.ll_bstride = a.ll_pitch * Hs;
			}
			const bool last = (j == 1);
			int ll_out = -1;
			if (last) {
				a.out = dst.p;
				a.out_pitch = dst.sx / es;
				a.out_bstride = dst_bstride / es;
				if (cur.p == dst.p) {
					// in place: the final level would overwrite subbands it still reads;
					// move them (right half + bottom-left, and LL if it is still there) aside
					if (batch != 1)
						return fail("in-place batches are not supported; use distinct src and dst");
					if (grow(g.stage_img, (size_t)dst.sx * Ho))
						return 1;
					Img st{(char *)g.stage_img.p, dst.sx, es};
					const Rect rc[3] = {{Ws, 0, Ws, 0, Wo - Ws, Ho}, {0, Hs, 0, Hs, Ws, Ho - Hs}, {0, 0, 0, 0, ll_in < 0 ? Ws : 0, Hs}};
					if (ride.on) {
						// (most of it went with the deeper levels' launches; what is left goes now)
						if (ride.flush())
							return 1;
					} else if (copy_staged(st, cur, rc, 3, /* temporal both ways: the final level reads the staged subbands (233 against 237 us) */ 0))
						return 1;
					a.in_h = st.p;
					a.h_bstride = 0;
					if (ll_in < 0)
						a.in_ll = st.p;
				}
			} else {
				ll_out = j & 1; // band of level m = j-1 lives in scratch (m-1)&1, as in the forward driver
				a.out = ll_band(ll_out);
				a.out_pitch = ll_pitch_elems(Wo);
				a.out_bstride = a.out_pitch * Ho;
				// (not for an in-place call: its staged subbands want the cache, 221 -> 224 us with both)
				a.temporal_out = g.tune.inv_ll_temporal && src.p != dst.p && (size_t)Wo * Ho * es * batch <= ((size_t)128 << 20);
			}
			SweepTuning tune = g.tune;
			if (tune.inv_pairs <= 0)
				tune.inv_pairs = src.p == dst.p ? 32 : 16; // (in place: 32 pairs, 230.7 against 234.0 us; scripts/r06/inv_call_ab.py)
			if (es == 4 && tune.tile_pairs <= 0)
				apply_tile_choice(tuned_tile_pairs(w, a), &tune, kTileInv);
			if (ride.on && !last && ride.next < ride.total && sweep_ride_ok(tune, Wo, Ho, batch, true)) {
				int after = 0;
				for (int m = j - 1; m >= 2; m--)
					after += sweep_ride_ok(g.tune, ge.Wo(m - 1), ge.Ho(m - 1), batch, true);
				a.ride = &ride.r;
				a.ride_lo = ride.next;
				a.ride_hi = ride.next + ride.share((size_t)Wo * Ho * es, after);
				ride.next = a.ride_hi;
			}
			prof_before(j - 1);
			hipError_t e = sweep_inv(c, a, tune, g.stream);
			prof_after(j - 1);
			if (e != hipSuccess)
				return fail("inverse level %d launch failed: %s", j, hipGetErrorString(e));
			ll_in = ll_out;
			continue;
		}

		// ---- generic level, in place on dst ----
		if (batch != 1)
			return fail("batched transforms need dense frames with both sides >= 2 at every level");
		if (src.p != dst.p && !copied) {
			// the `_s2` entry copies the inner region, then works in place (:18001-18008)
			if (copy_rect(dst, 0, 0, src, 0, 0, ge.six, ge.siy))
				return 1;
			copied = true;
		}
		cur = dst;
		cur_bstride = dst_bstride;
		if (ll_in >= 0) {
			// a deeper fused level left its result in scratch: bring it back into the image
			Img s{ll_band(ll_in), ll_pitch_elems(Ws) * es, es};
			if (copy_rect(dst, 0, 0, s, 0, 0, Ws, Hs))
				return 1;
			ll_in = -1;
		}
		if (generic_level(c, true, dst, dst, Wo, Ho, Wi, Hi, Ws, Hs))
			return 1;
		if (zero_padding) {
			// dwt_zero_padding_i_stride_* (src/libdwt.c:12161-12215)
			if (zero_rect(dst, Wi, 0, Wo - Wi, Ho) || zero_rect(dst, 0, Hi, Wo, Ho - Hi))
				return 1;
		}
	}
	return 0;
}

int check_inited()
{
	if (!g.inited && dwt_hip_init())
		return 1;
	return 0;
}

} // namespace dwtb
