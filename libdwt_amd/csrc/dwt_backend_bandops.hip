// dwt_backend_bandops.hip -- the per-band coefficient operators (thresholds, scaling, tone compression, zeroing), the
// pointwise log / exp maps and the universal threshold estimate on the device, and their C-ABI (include/libdwt_hip.h;
// DESIGN.md s17).
//
// The slots of a frame decomposed to J levels are the bands of dwt_util_subband_s (src/libdwt.c:20731) over its outer and
// inner sizes: slot 3(j-1) + {0, 1, 2} is HL, LH, HH of level j = 1 .. J, slot 3J is LL of level J; empty bands keep their
// slot.  The geometry, the prefix of the slots' chunk counts and the operator table travel as kernel arguments, so that a
// call is ONE launch (dwt_bandops.hip) and nothing else: no allocation, no copy.  Per-image tables of a batch
// (table_stride != 0) cannot ride in the arguments; they are copied to the context's band workspace first.  Dense device
// frames run where they lie; host memory and device frames whose elements are not adjacent go through the staging path
// of every other driver (frame_pack_stack / frame_unpack_stack: only the frame's own elements are written back).
#include "dwt_backend.h"

#include <climits>
#include <cmath>

namespace dwtb {

namespace {

inline long cdiv_pow2(long i, int j) { return (i + (1l << j) - 1) >> j; }

// The level count a call works with.  j_max < 0: as many levels as the transforms give these sizes by default
// (decompose_one = 0: the smaller side; a single row or column: its length, the 1-D transforms' rule).  Otherwise j_max,
// at most what any transform can return for these sizes (decompose_one = 1: the larger side).
int levels_of(int sox, int soy, int j_max)
{
	const int lo = std::min(sox, soy), hi = std::max(sox, soy);
	if (j_max < 0)
		return ceil_log2(lo <= 1 ? hi : lo);
	return std::min(j_max, ceil_log2(hi));
}

// slot geometry of a frame; returns the number of slots (3J + 1)
int fill_slots(const Geom &ge, int J, BandOpsArgs *a)
{
	auto put = [&](int k, long x0, long y0, long w, long h) {
		a->x0[k] = (int)x0;
		a->y0[k] = (int)y0;
		a->w[k] = (int)w;
		a->h[k] = (int)h;
	};
	for (int j = 1; j <= J; j++) {
		const long hx = cdiv_pow2(ge.six, j - 1) / 2, hy = cdiv_pow2(ge.siy, j - 1) / 2, lx = cdiv_pow2(ge.six, j), ly = cdiv_pow2(ge.siy, j);
		const long ox = cdiv_pow2(ge.sox, j), oy = cdiv_pow2(ge.soy, j);
		put(3 * (j - 1) + 0, ox, 0, hx, ly);
		put(3 * (j - 1) + 1, 0, oy, lx, hy);
		put(3 * (j - 1) + 2, ox, oy, hx, hy);
	}
	put(3 * J, 0, 0, cdiv_pow2(ge.six, J), cdiv_pow2(ge.siy, J));
	return 3 * J + 1;
}

long chunks_of(int w, int h)
{
	if (w <= 0 || h <= 0)
		return 0;
	const int cw = band_chunk_cols(w), rh = band_chunk_rows(w);
	return (long)((w + cw - 1) / cw) * ((h + rh - 1) / rh);
}

// The table of `n_tables` images (1: shared by the batch), image t's at ops + t*tstride: checked, entered into the
// arguments -- the shared table itself, or the per-image tables through the band workspace -- and the prefix of the chunk
// counts built over the slots at least one image touches.  op_lo .. op_hi: the operators this entry takes.
int fill_table(BandOpsArgs *a, const int *ops, const float *params, int n_tables, long tstride, int op_lo, int op_hi)
{
	const int ns = a->nslots;
	bool touched[BAND_MAX_SLOTS] = {};
	for (int t = 0; t < n_tables; t++)
		for (int k = 0; k < ns; k++) {
			const int op = ops[(long)t * tstride + k];
			if (op != kBandKeep && (op < op_lo || op > op_hi))
				return fail("unknown operator %d in slot %d of table %d", op, k, t);
			touched[k] = touched[k] || op != kBandKeep;
		}
	long first = 0;
	for (int k = 0; k < ns; k++) {
		a->first[k] = (int)first;
		if (touched[k])
			first += chunks_of(a->w[k], a->h[k]);
		if (first > INT_MAX)
			return fail("frame too large for one launch (%ld chunks)", first);
	}
	a->first[ns] = (int)first;
	a->dev_op = nullptr;
	a->dev_param = nullptr;
	a->tstride = 0;
	if (n_tables == 1) {
		for (int k = 0; k < ns; k++) {
			a->op[k] = (unsigned char)ops[k];
			a->param[k] = params[k];
		}
		return 0;
	}
	if (first == 0)
		return 0;
	// per-image tables, packed: ints, then floats (pageable memory: the copies have read it when they return)
	const size_t n = (size_t)n_tables * ns;
	if (grow(g.band_ws, n * 8))
		return 1;
	static thread_local std::vector<int> packed;
	packed.resize(2 * n);
	for (int t = 0; t < n_tables; t++)
		for (int k = 0; k < ns; k++) {
			packed[(size_t)t * ns + k] = ops[(long)t * tstride + k];
			memcpy(&packed[n + (size_t)t * ns + k], &params[(long)t * tstride + k], 4);
		}
	HIP_TRY(hipMemcpyAsync(g.band_ws.p, packed.data(), n * 8, hipMemcpyHostToDevice, g.stream));
	a->dev_op = (const int *)g.band_ws.p;
	a->dev_param = (const float *)g.band_ws.p + n;
	a->tstride = ns;
	return 0;
}

// The launch over `batch` frames of fw x fh elements, frame b at ptr + b*bstride, rows sx bytes apart, elements sy: dense
// device frames where they lie, everything else through the staging path.  *a holds geometry and table.
int run_frames(void *ptr, long bstride, int batch, long sx, long sy, int fw, int fh, BandOpsArgs *a)
{
	if (batch == 0 || fw == 0 || fh == 0 || a->first[a->nslots] == 0)
		return 0; // (an all-KEEP table launches nothing and moves nothing)
	const bool dev = dwt_hip_is_device_pointer(ptr);
	if (dev && check_dev_align({ptr}, {sx, sy, bstride}))
		return 1;
	if (fh == 1)
		sx = sy * fw; // (one row: its stride is never used)
	a->batch = batch;
	if (dev && sy == 4) {
		a->img = (char *)ptr;
		a->pitch = sx;
		a->bstride = bstride;
		return launched(launch_band_ops(*a, g.stream), "band", "operator");
	}
	const long pitch = frame_pitch(4, fw);
	if (grow(g.frame_a, (size_t)pitch * fh * batch))
		return 1;
	const Frame fr{ptr, sx, sy, 4, fw, fh, dev};
	a->img = (char *)g.frame_a.p;
	a->pitch = pitch;
	a->bstride = pitch * fh;
	if (frame_pack_stack(fr, batch, bstride, g.frame_a.p, pitch) || launched(launch_band_ops(*a, g.stream), "band", "operator"))
		return 1;
	return frame_unpack_stack(fr, batch, bstride, g.frame_a.p, pitch);
}

int check_frames(const void *ptr, long bstride, int batch, long sx, long sy, int sox, int soy, int six, int siy)
{
	if (!ptr)
		return fail("null pointer argument");
	if (batch < 0 || sox < 0 || soy < 0 || six < 0 || siy < 0 || six > sox || siy > soy)
		return fail("bad sizes: outer %d x %d, inner %d x %d, batch %d", sox, soy, six, siy, batch);
	if (sy < 4 || (soy > 1 && sx < sy * (long)sox))
		return fail("bad strides: %ld, %ld bytes", sx, sy);
	if (batch > 1 && bstride < (soy > 1 ? sx * (long)soy : sy * (long)sox))
		return fail("frames must be apart (batch stride %ld)", bstride);
	return 0;
}

int bands_apply(void *ptr, long bstride, int batch, long sx, long sy, int sox, int soy, int six, int siy, int j_max, const int *ops,
	const float *params, size_t table_stride)
{
	if (check_inited() || check_frames(ptr, bstride, batch, sx, sy, sox, soy, six, siy))
		return 1;
	if (!ops || !params)
		return fail("null operator table");
	if (table_stride > (size_t)INT_MAX)
		return fail("bad table stride %zu", table_stride);
	const Geom ge{sox, soy, six, siy};
	BandOpsArgs a{};
	a.nslots = fill_slots(ge, levels_of(sox, soy, j_max), &a);
	if (table_stride && table_stride < (size_t)a.nslots)
		return fail("table stride %zu, one table takes %d entries", table_stride, a.nslots);
	const int n_tables = table_stride && batch > 0 ? batch : 1;
	if (fill_table(&a, ops, params, n_tables, (long)table_stride, kBandZero, kBandCompress))
		return 1;
	return run_frames(ptr, bstride, batch, sx, sy, sox, soy, &a);
}

int map_frames(int op, void *ptr, long bstride, int batch, long sx, long sy, int size_x, int size_y, float prm)
{
	if (op != DWT_HIP_MAP_LOG && op != DWT_HIP_MAP_EXP)
		return fail("unknown map %d", op);
	if (check_inited() || check_frames(ptr, bstride, batch, sx, sy, size_x, size_y, size_x, size_y))
		return 1;
	BandOpsArgs a{};
	a.nslots = fill_slots(Geom{size_x, size_y, size_x, size_y}, 0, &a); // the whole frame as its one band
	const int kop = op == DWT_HIP_MAP_LOG ? kMapLog : kMapExp;
	if (fill_table(&a, &kop, &prm, 1, 0, kMapLog, kMapExp))
		return 1;
	return run_frames(ptr, bstride, batch, sx, sy, size_x, size_y, &a);
}

} // namespace

} // namespace dwtb

using namespace dwtb;

#pragma GCC visibility push(default)
extern "C" {

int dwt_hip_band_levels(int size_o_x, int size_o_y, int j_max)
{
	if (size_o_x < 0 || size_o_y < 0)
		return -1;
	return levels_of(size_o_x, size_o_y, j_max);
}

int dwt_hip_band_slots(int j_max) { return j_max < 0 || j_max > 31 ? -1 : 3 * j_max + 1; }

int dwt_hip_band_geometry(int size_o_x, int size_o_y, int size_i_x, int size_i_y, int j_max, int *xywh)
{
	if (size_o_x < 0 || size_o_y < 0 || size_i_x < 0 || size_i_y < 0 || size_i_x > size_o_x || size_i_y > size_o_y || !xywh)
		return -1;
	BandOpsArgs a{};
	const int ns = fill_slots(Geom{size_o_x, size_o_y, size_i_x, size_i_y}, levels_of(size_o_x, size_o_y, j_max), &a);
	for (int k = 0; k < ns; k++) {
		xywh[4 * k] = a.x0[k];
		xywh[4 * k + 1] = a.y0[k];
		xywh[4 * k + 2] = a.w[k];
		xywh[4 * k + 3] = a.h[k];
	}
	return ns;
}

int dwt_hip_bands_apply(void *ptr, int stride_x, int stride_y, int size_o_x, int size_o_y, int size_i_x, int size_i_y, int j_max,
	const int *ops, const float *params)
{
	return bands_apply(ptr, 0, 1, stride_x, stride_y, size_o_x, size_o_y, size_i_x, size_i_y, j_max, ops, params, 0);
}

int dwt_hip_bands_apply_batch(void *ptr, size_t batch_stride, int batch, int stride_x, int size_x, int size_y, int j_max, const int *ops,
	const float *params, size_t table_stride)
{
	if (batch_stride > (size_t)LONG_MAX / 2)
		return fail("bad batch stride %zu", batch_stride);
	return bands_apply(ptr, (long)batch_stride, batch, stride_x, 4, size_x, size_y, size_x, size_y, j_max, ops, params, table_stride);
}

int dwt_hip_map(int op, void *ptr, int stride_x, int stride_y, int size_x, int size_y, float a)
{
	return map_frames(op, ptr, 0, 1, stride_x, stride_y, size_x, size_y, a);
}

int dwt_hip_map_batch(int op, void *ptr, size_t batch_stride, int batch, int stride_x, int size_x, int size_y, float a)
{
	if (batch_stride > (size_t)LONG_MAX / 2)
		return fail("bad batch stride %zu", batch_stride);
	return map_frames(op, ptr, (long)batch_stride, batch, stride_x, 4, size_x, size_y, a);
}

int dwt_hip_universal_threshold_batch(const void *ptr, size_t batch_stride, int batch, int stride_x, int size_x, int size_y, float *lambda)
{
	if (batch_stride > (size_t)LONG_MAX / 2)
		return fail("bad batch stride %zu", batch_stride);
	if (check_inited() || check_frames(ptr, (long)batch_stride, batch, stride_x, 4, size_x, size_y, size_x, size_y))
		return 1;
	if (!lambda || dwt_hip_is_device_pointer(lambda))
		return fail("the thresholds go to host memory");
	if (batch == 0)
		return 0;
	const int w = size_x / 2, h = size_y / 2; // HH(1)
	if (w == 0 || h == 0)
		return fail("a frame of %d x %d has no HH(1) band", size_x, size_y);
	if (band_abs_median(ptr, (long)batch_stride, batch, stride_x, size_x, size_y, size_x - w, size_y - h, w, h, lambda))
		return 1;
	// denoise_estimate_threshold (src/denoise.c:71-73), in float as the reference writes it
	const float spread = sqrtf(2.f * logf((float)((long)size_x * size_y)));
	for (int b = 0; b < batch; b++) {
		const float sigma = lambda[b] / 0.6745f;
		lambda[b] = sigma * spread;
	}
	return 0;
}

} // extern "C"
#pragma GCC visibility pop
