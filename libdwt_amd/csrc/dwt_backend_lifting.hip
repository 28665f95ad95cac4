// dwt_backend_lifting.hip -- user-defined lifting wavelets: the multi-level Mallat driver of a batch of dense frames and
// its C-ABI (include/libdwt_hip.h).  The scheme is checked by dwt_lifting_scheme.c (plain C), turned into
// the kernels' table here and rides in the kernel arguments.
//
// FUSED (reach <= 8, option "lifting_fused" != 0): one launch of the tile kernel per level for the whole batch.  The
// forward's level 0 reads the source, deeper levels the LL ping-pong of the context; every level writes its detail bands to
// the destination and its LL to the ping-pong, the last one to the destination.  The inverse reads every level's detail
// bands from the source and passes LL through the ping-pong; level 1 writes the destination.  src == dst: the tiles would
// read halos that other tiles have overwritten, so the batch is copied into scratch first (one more launch) and that copy
// is the source.
// STEPS: per level a dense copy of the LL rectangle (forward) or the gathered subbands (inverse) in scratch, one
// elementwise launch per step and direction in place there, and one launch that places the result.  Any size, any reach.
// Host memory and strided device frames are packed into a dense device stack first, as the other drivers do.
//
// Line batches (dwt_hip_lifting1d_batch): every level whose line has at most N1D_MAX samples in ONE launch
// of k_lift_lines, straight from src to dst, any reach.  Option "lifting_fused" = 0, and the leading levels of longer
// lines, go level by level through the dense scratch (frame_b) with one launch per step -- the split of dwt_backend_1d.hip.
#include "dwt_backend.h"

#include <climits>

namespace dwtb {

namespace {

static_assert(LIFT_MAX_STEPS == DWT_HIP_LIFT_MAX_STEPS && LIFT_MAX_TERMS == DWT_HIP_LIFT_MAX_TERMS && LIFT_FUSED_REACH == DWT_HIP_LIFT_FUSED_REACH,
	"the header states the kernels' constants");

// the checked scheme as the kernels take it
int table_of(const dwt_hip_lifting *s, LiftTable *tb)
{
	int reach = 0;
	if (dwt_hip_lifting_check(s, &reach))
		return 1;
	*tb = LiftTable{};
	tb->is_int = s->type == DWT_HIP_LIFT_I32;
	tb->n_steps = s->n_steps;
	tb->inv_cols_first = s->inverse_cols_first;
	tb->reach = reach;
	for (int p = 0; p < 2; p++) {
		tb->fwd_scale[p] = tb->is_int ? 1.0f : s->fwd_scale[p];
		tb->inv_scale[p] = tb->is_int ? 1.0f : s->inv_scale[p];
	}
	for (int k = 0; k < s->n_steps; k++) {
		const dwt_hip_lifting_step &in = s->steps[k];
		LiftStep &st = tb->steps[k];
		st.parity = in.parity, st.n_terms = in.n_terms;
		st.sign = in.sign, st.add = in.add, st.shift = in.shift;
		for (int t = 0; t < in.n_terms; t++) {
			st.off_a[t] = in.terms[t].off_a, st.off_b[t] = in.terms[t].off_b;
			st.coef[t] = in.terms[t].coef, st.num[t] = in.terms[t].num;
			st.reach = std::max({st.reach, abs(in.terms[t].off_a), abs(in.terms[t].off_b)});
		}
	}
	return 0;
}

bool fused_route(const LiftTable &tb) { return g.lifting_fused != 0 && tb.reach <= LIFT_FUSED_REACH; }

struct Frames {
	int W, H, batch, J;
	long pitch, bs; // of src and dst alike, in elements
	int Wo(int j) const { return ceil_div_pow2(W, j); }
	int Ho(int j) const { return ceil_div_pow2(H, j); }
};

int copy_frames(const void *src, long ps, long bs, void *dst, long pd, long bd, int W, int H, int batch)
{
	return launched(launch_lift_copy(src, ps, bs, dst, pd, bd, W, H, batch, g.stream), "lifting", "copy");
}

int run_fused(bool inverse, const LiftTable &tb, const Frames &f, const char *src, char *dst)
{
	const int J = f.J;
	const long pll = f.Wo(1), bll = (long)f.Wo(1) * f.Ho(1);
	const void *s = src;
	long ps = f.pitch, sbs = f.bs;
	if (src == dst) { // the copy that the tiles read
		if (grow(g.frame_b, (size_t)f.W * f.H * 4 * f.batch))
			return 1;
		if (copy_frames(src, f.pitch, f.bs, g.frame_b.p, f.W, (long)f.W * f.H, f.W, f.H, f.batch))
			return 1;
		s = g.frame_b.p, ps = f.W, sbs = (long)f.W * f.H;
	}
	void *LL[2] = {nullptr, nullptr};
	for (int k = 0; k < 2 && k < J - 1; k++) {
		if (grow(g.lift_ll[k], (size_t)bll * 4 * f.batch))
			return 1;
		LL[k] = g.lift_ll[k].p;
	}
	for (int n = 0; n < J; n++) {
		LiftLevelArgs a;
		a.batch = f.batch;
		a.det = inverse ? const_cast<void *>(s) : (void *)dst; // (the inverse only reads it)
		a.pd = inverse ? ps : f.pitch, a.bi_det = inverse ? sbs : f.bs;
		const bool first = n == 0, last = n == J - 1;
		a.in = first ? s : LL[(n - 1) & 1], a.pin = first ? ps : pll, a.bi_in = first ? sbs : bll;
		a.out = last ? (void *)dst : LL[n & 1], a.pout = last ? f.pitch : pll, a.bi_out = last ? f.bs : bll;
		const int j = inverse ? J - 1 - n : n; // the level whose rectangle this launch works on
		a.W = f.Wo(j), a.H = f.Ho(j);
		if (launched(launch_lift_tile(inverse, tb, a, g.stream), "lifting", "level"))
			return 1;
	}
	return 0;
}

// every step of one direction on the dense scratch, in the order of the direction of the transform
int steps_pass(bool inverse, const LiftTable &tb, void *x, int W, int H, int batch, bool rows)
{
	if ((rows ? W : H) < 2)
		return 0;
	for (int si = 0; si < tb.n_steps; si++)
		if (launched(launch_lift_step(tb.is_int, inverse, x, W, H, batch, tb.steps[inverse ? tb.n_steps - 1 - si : si], rows, g.stream), "lifting", "step"))
			return 1;
	return 0;
}

int run_steps(bool inverse, const LiftTable &tb, const Frames &f, const char *src, char *dst)
{
	if (grow(g.frame_b, (size_t)f.W * f.H * 4 * f.batch))
		return 1;
	void *x = g.frame_b.p;
	const float *fs = inverse ? tb.inv_scale : tb.fwd_scale;
	const bool scale = !tb.is_int && (fs[0] != 1.0f || fs[1] != 1.0f);
	for (int n = 0; n < f.J; n++) {
		const int j = inverse ? f.J - 1 - n : n;
		const int W = f.Wo(j), H = f.Ho(j);
		const void *ll = n == 0 ? (const void *)src : (const void *)dst; // where the level's LL rectangle lies
		if (!inverse) {
			if (copy_frames(ll, f.pitch, f.bs, x, W, (long)W * H, W, H, f.batch) || steps_pass(false, tb, x, W, H, f.batch, true))
				return 1;
			if (scale && launched(launch_lift_scale(x, W, H, f.batch, true, fs[0], fs[1], g.stream), "lifting", "scale"))
				return 1;
			if (steps_pass(false, tb, x, W, H, f.batch, false) ||
			    launched(launch_lift_place(x, dst, f.pitch, f.bs, W, H, f.batch, scale, fs[0], fs[1], g.stream), "lifting", "place"))
				return 1;
			continue;
		}
		const bool rows_first = !tb.inv_cols_first;
		if (launched(launch_lift_gather(ll, f.pitch, f.bs, src, f.pitch, f.bs, x, W, H, f.batch, scale, rows_first, fs[0], fs[1], g.stream), "lifting", "gather") ||
		    steps_pass(true, tb, x, W, H, f.batch, rows_first))
			return 1;
		if (scale && launched(launch_lift_scale(x, W, H, f.batch, !rows_first, fs[0], fs[1], g.stream), "lifting", "scale"))
			return 1;
		if (steps_pass(true, tb, x, W, H, f.batch, !rows_first) || copy_frames(x, W, (long)W * H, dst, f.pitch, f.bs, W, H, f.batch))
			return 1;
	}
	return 0;
}

// dense device frames, src == dst or apart
int run_device(bool inverse, const LiftTable &tb, const Frames &f, const char *src, char *dst)
{
	if (f.J == 0) // no level: the frames as they are
		return src == dst ? 0 : copy_frames(src, f.pitch, f.bs, dst, f.pitch, f.bs, f.W, f.H, f.batch);
	return fused_route(tb) ? run_fused(inverse, tb, f, src, dst) : run_steps(inverse, tb, f, src, dst);
}

// ---- a batch of lines (dwt_hip_lifting1d_batch) -------------------------------------------------------------

struct Lines {
	int N, n_lines, J;
	long ls, es; // of src and dst alike, in WORDS
	int len(int j) const { return ceil_div_pow2(N, j); }
};

// levels whose line is longer than the fused kernel takes (the split of dwt_backend_1d.hip)
int lines_long_levels(int N, int J)
{
	int j = 0;
	while (j < J && ceil_div_pow2(N, j) > N1D_MAX)
		j++;
	return j;
}

bool lines_fused_route(int size) { return g.lifting_fused != 0 && size <= N1D_MAX; }

int line_move(int mode, const void *ll, const void *det, long sls, long ses, void *dst, long dls, long des, int W, int H, bool scale, const float *fs)
{
	return launched(launch_lift_line_move(mode, ll, det, sls, ses, dst, dls, des, W, H, scale, fs[0], fs[1], g.stream), "lifting", "line move");
}

// Level j of every line step by step: the level's prefix of the lines into the dense scratch (a frame of W = the prefix, H
// = n_lines, lifted along rows only), one launch per step there, the result back to dst's prefix.  Forward: the prefix of
// `ll` in sample order -> Mallat order.  Inverse: L from `ll`, H from `det` -> sample order.
int lines_steps_level(bool inverse, const LiftTable &tb, const Lines &l, int j, const char *ll, const char *det, char *dst)
{
	const int W = l.len(j), H = l.n_lines;
	void *x = g.frame_b.p;
	const float *fs = inverse ? tb.inv_scale : tb.fwd_scale;
	const bool scale = !tb.is_int && (fs[0] != 1.0f || fs[1] != 1.0f);
	if (line_move(inverse ? 1 : 0, ll, det, l.ls, l.es, x, W, 1, W, H, scale, fs) || steps_pass(inverse, tb, x, W, H, 1, true))
		return 1;
	return line_move(inverse ? 0 : 2, x, x, W, 1, dst, l.ls, l.es, W, H, scale, fs);
}

// device lines whose addresses and strides are multiples of 4 bytes, src == dst or apart
int run_lines(bool inverse, const LiftTable &tb, const Lines &l, const char *src, char *dst)
{
	const int J = l.J;
	if (J == 0) // no level: the lines as they are
		return src == dst ? 0 : line_move(0, src, src, l.ls, l.es, dst, l.ls, l.es, l.N, l.n_lines, false, tb.fwd_scale);
	const int jg = g.lifting_fused != 0 ? lines_long_levels(l.N, J) : J; // levels 0 .. jg-1 step by step
	if (jg > 0 && grow(g.frame_b, (size_t)l.N * 4 * l.n_lines))
		return 1;
	auto fused = [&](const char *s) {
		return launched(launch_lift_lines(inverse, tb, s, dst, l.ls * 4, l.es * 4, l.n_lines, l.len(jg), J - jg, g.stream), "lifting", "lines");
	};
	if (!inverse) {
		for (int j = 0; j < jg; j++)
			if (lines_steps_level(false, tb, l, j, j == 0 ? src : dst, nullptr, dst))
				return 1;
		return jg < J ? fused(jg == 0 ? src : dst) : 0;
	}
	// (the inverse reads every H band from src; what a level has rebuilt lies in dst)
	if (jg < J && fused(src))
		return 1;
	for (int j = jg - 1; j >= 0; j--)
		if (lines_steps_level(true, tb, l, j, j == J - 1 ? src : dst, src, dst))
			return 1;
	return 0;
}

} // namespace

} // namespace dwtb

using namespace dwtb;

// the error text of dwt_lifting_scheme.c's refusals
extern "C" void dwt_lifting_set_error(const char *msg) { fail("%s", msg); }

#pragma GCC visibility push(default)
extern "C" {

int dwt_hip_lifting2d_batch(const struct dwt_hip_lifting *scheme, int inverse, const void *src, void *dst, size_t batch_stride, int batch,
	int stride_x, int stride_y, int size_x, int size_y, int *j)
{
	LiftTable tb;
	if (table_of(scheme, &tb))
		return 1;
	if (!src || !dst || !j)
		return fail("null pointer argument");
	if (size_x < 1 || size_y < 1 || (long)size_x * size_y > INT_MAX)
		return fail("lifting: bad sizes %d x %d (at least 1 x 1, at most INT_MAX samples)", size_x, size_y);
	if (batch < 1 || batch > DWT_HIP_LIFT_MAX_BATCH)
		return fail("lifting: %d frames (1 .. %d)", batch, DWT_HIP_LIFT_MAX_BATCH);
	const long sx = stride_x, sy = stride_y;
	if (sy < 4 || (size_y > 1 && sx < sy * size_x))
		return fail("lifting: bad strides: %d, %d bytes", stride_x, stride_y);
	const long one = size_y > 1 ? sx * (size_y - 1) + sy * (size_x - 1) + 4 : sy * (size_x - 1) + 4; // bytes a frame spans
	if (batch_stride > (size_t)LONG_MAX / DWT_HIP_LIFT_MAX_BATCH || (batch > 1 && (long)batch_stride < one))
		return fail("lifting: frames must be apart (batch stride %zu bytes, a frame spans %ld)", batch_stride, one);
	const long bstride = batch > 1 ? (long)batch_stride : 0;
	const size_t extent = (size_t)bstride * (batch - 1) + one;
	if (src != dst && overlap(src, extent, dst, extent))
		return fail("lifting: src and dst overlap (src == dst is the in-place call)");
	if (check_inited())
		return 1;
	const bool dev = dwt_hip_is_device_pointer(src);
	if (dev != (bool)dwt_hip_is_device_pointer(dst))
		return fail("lifting: src and dst must both be host or both be device memory");
	if (dev && check_dev_align({src, dst}, {sx, sy, bstride}))
		return 1;
	Frames f;
	f.W = size_x, f.H = size_y, f.batch = batch;
	f.J = dwt_hip_band_levels(size_x, size_y, *j);
	if (f.J < 0 || f.J > 31)
		return fail("lifting: bad level count for %d x %d", size_x, size_y);
	*j = f.J;
	if (dev && sy == 4) {
		f.pitch = size_y > 1 ? sx / 4 : size_x, f.bs = bstride / 4;
		return run_device(inverse != 0, tb, f, (const char *)src, (char *)dst);
	}
	// host memory, strided device frames: the staging detour (dwt_backend.h), in place on the dense stack
	const long pitch = frame_pitch(4, size_x);
	if (size_y == 1)
		stride_x = (int)(sy * size_x); // (one row: its stride is never used)
	const Frame fs{const_cast<void *>(src), stride_x, sy, 4, size_x, size_y, dev}, fd{dst, stride_x, sy, 4, size_x, size_y, dev};
	if (frame_check(fs) || grow(g.frame_a, (size_t)pitch * size_y * batch))
		return 1;
	f.pitch = pitch / 4, f.bs = pitch / 4 * size_y;
	if (frame_pack_stack(fs, batch, bstride, g.frame_a.p, pitch) || run_device(inverse != 0, tb, f, (const char *)g.frame_a.p, (char *)g.frame_a.p))
		return 1;
	return frame_unpack_stack(fd, batch, bstride, g.frame_a.p, pitch);
}

int dwt_hip_lifting_route(const struct dwt_hip_lifting *scheme)
{
	LiftTable tb;
	if (table_of(scheme, &tb))
		return -1;
	return fused_route(tb) ? DWT_HIP_LIFT_FUSED : DWT_HIP_LIFT_STEPS;
}

int dwt_hip_lifting1d_batch(const struct dwt_hip_lifting *scheme, int inverse, const void *src, void *dst, size_t line_stride, int elem_stride,
	int n_lines, int size, int *j)
{
	LiftTable tb;
	if (table_of(scheme, &tb))
		return 1;
	if (!src || !dst || !j)
		return fail("null pointer argument");
	if (size < 1)
		return fail("lifting: bad sizes: %d samples a line (at least 1)", size);
	if (n_lines < 1)
		return fail("lifting: %d lines (at least 1)", n_lines);
	const long es = elem_stride;
	const long one = es * (size - 1) + 4; // bytes a line spans
	if (es < 4 || line_stride > (size_t)LONG_MAX / 2 / (size_t)n_lines || (n_lines > 1 && (long)line_stride < one))
		return fail("lifting: bad strides: line %zu bytes, element %d bytes", line_stride, elem_stride);
	const long ls = n_lines > 1 ? (long)line_stride : 0;
	const size_t extent = (size_t)ls * (n_lines - 1) + one;
	if (src != dst && overlap(src, extent, dst, extent))
		return fail("lifting: src and dst overlap (src == dst is the in-place call)");
	if (check_inited())
		return 1;
	const bool dev = dwt_hip_is_device_pointer(src);
	if (dev != (bool)dwt_hip_is_device_pointer(dst))
		return fail("lifting: src and dst must both be host or both be device memory");
	// the level count, clamped as transform1d (dwt_backend_1d.hip) clamps it
	const int j_limit = ceil_log2(size);
	Lines l;
	l.N = size, l.n_lines = n_lines;
	if (!inverse) {
		if (*j < 0 || *j > j_limit)
			*j = j_limit;
		l.J = *j;
	} else {
		l.J = *j >= 0 && *j < j_limit ? *j : j_limit;
	}
	if (l.J == 0 && src == dst)
		return 0;
	if (dev && es % 4 == 0 && ls % 4 == 0 && (uintptr_t)src % 4 == 0 && (uintptr_t)dst % 4 == 0) {
		l.ls = ls / 4, l.es = es / 4;
		return run_lines(inverse != 0, tb, l, (const char *)src, (char *)dst);
	}
	// host memory, device lines that are not made of aligned words: the staging detour (dwt_backend.h), in place on the dense frame
	const Frame fs{const_cast<void *>(src), ls ? ls : one, es, 4, size, n_lines, dev};
	if (frame_check(fs))
		return 1;
	Img A;
	if (frame_stage(fs, g.frame_a, &A))
		return 1;
	l.ls = A.sx / 4, l.es = 1;
	if (run_lines(inverse != 0, tb, l, A.p, A.p))
		return 1;
	return frame_unpack(Frame{dst, fs.sx, es, 4, size, n_lines, dev}, A.p, A.sx);
}

int dwt_hip_lifting1d_route(const struct dwt_hip_lifting *scheme, int size)
{
	LiftTable tb;
	if (table_of(scheme, &tb))
		return -1;
	if (size < 1) {
		fail("lifting: bad sizes: %d samples a line (at least 1)", size);
		return -1;
	}
	return lines_fused_route(size) ? DWT_HIP_LIFT_FUSED : DWT_HIP_LIFT_STEPS;
}

} // extern "C"
#pragma GCC visibility pop
