// dwt_backend_bitplane.hip -- embedded bit-plane streams of code-blocks: the blocks of int16 / int32 index planes packed
// into sign and magnitude planes of 64-bit words in stream order, and unpacked with the least significant planes left
// out on request; their C-ABI (include/libdwt_hip.h).
//
// Pack is three launches of dwt_bitplane.hip on the context's stream -- the blocks' sizes, the scan of one workgroup per
// frame, the words --, count only the first two, unpack one.  The band table in stream order and its blocks come from
// dwt_bitplane_geom.c and ride in the kernel arguments; the blocks' sizes live in the context's workspace.  Each of the
// three sides -- the planes, the words, the offsets -- lies in host or in device memory on its own; a host side is
// mirrored like a side of the quantizer (mirror / mirror_back).
#include "dwt_backend.h"

#include <climits>

namespace dwtb {

namespace {

static_assert(BITPLANE_GRID_BLOCKS == DWT_HIP_BITPLANE_GRID_BLOCKS && BITPLANE_GRID_BATCH == DWT_HIP_BITPLANE_GRID_BATCH &&
		(int)kBitplaneKeep == DWT_HIP_BITPLANE_KEEP && (int)kBitplaneShift == DWT_HIP_BITPLANE_SHIFT, "the header states the kernels' constants");

// the frames of a call: `batch` frames of W x H indices of es bytes, their bands in stream order and their blocks
struct Frames {
	int index_type, batch, W, H, es, bands, cbx, cby;
	long pitch, bs; // (a stride that no element is reached by is 0)
	Side side;
	int table[5 * (BAND_MAX_SLOTS + 1)];
	int blocks() const { return table[5 * bands + 4]; }
	bool empty() const { return batch == 0 || W == 0 || H == 0; }
};

int frames_check(Frames *f, int index_type, const void *p, size_t bs, size_t pitch, int batch, int W, int H, int j_max, int cbx, int cby)
{
	if (index_type != DWT_HIP_INDEX_I16 && index_type != DWT_HIP_INDEX_I32)
		return fail("bit-planes: unknown index type %d", index_type);
	f->index_type = index_type, f->es = quant_index_es(index_type);
	if (batch < 0 || W < 0 || H < 0 || (long)W * H > INT_MAX)
		return fail("bit-planes: bad sizes (%d frames of %d x %d; a frame holds at most INT_MAX elements)", batch, W, H);
	if (cbx < 2 || cbx > 10 || cby < 2 || cby > 10 || cbx + cby > 12)
		return fail("bit-planes: code-blocks of 2^%d x 2^%d samples (each exponent 2 .. 10, their sum at most 12)", cbx, cby);
	if (!p)
		return fail("null pointer argument");
	f->batch = batch, f->W = W, f->H = H, f->cbx = cbx, f->cby = cby;
	f->bands = dwt_hip_bitplane_bands(W, H, j_max, cbx, cby, f->table);
	if (f->bands != 3 * dwt_hip_band_levels(W, H, j_max) + 1)
		return fail("bit-planes: bad sizes (%d x %d, j_max %d)", W, H, j_max);
	const int es = f->es;
	const size_t lim = (size_t)1 << 46;
	if (bs > lim || pitch > lim)
		return fail("bit-planes: bad strides of the planes");
	f->bs = batch > 1 ? (long)bs : 0, f->pitch = H > 1 ? (long)pitch : 0;
	if ((uintptr_t)p % es || f->bs % es || f->pitch % es)
		return fail("bit-planes: the planes' address and strides are multiples of the element size (%d bytes)", es);
	const long row = (long)W * es;
	long one = row;
	if ((H > 1 && f->pitch < row) || !mul_add(&one, std::max(H - 1, 0), f->pitch))
		return fail("bit-planes: bad row pitch of the planes (%zu bytes for %d elements of %d)", pitch, W, es);
	if (batch > 1 && f->bs < one)
		return fail("bit-planes: the planes' frames must be apart (batch stride %zu bytes, a frame takes %ld)", bs, one);
	long extent = one;
	if (!mul_add(&extent, std::max(batch - 1, 0), f->bs))
		return fail("bit-planes: bad strides of the planes");
	f->side = Side{p, f->empty() ? 0 : (size_t)extent, (H < 2 || f->pitch == row) && (batch < 2 || f->bs == one)};
	return 0;
}

// a dense array of `batch` runs of `stride` elements of es bytes (the words, the offsets)
int array_check(Side *s, const char *what, const void *p, size_t stride, int es, int batch)
{
	if (!p)
		return fail("null pointer argument");
	if ((uintptr_t)p % es)
		return fail("bit-planes: the address of the %s is a multiple of %d bytes", what, es);
	if (stride > ((size_t)1 << 40))
		return fail("bit-planes: bad stride of the %s (%zu)", what, stride);
	*s = Side{p, (size_t)batch * stride * es, true};
	return 0;
}

// the regions of a call must not share a byte
int apart(const Frames &f, const Side &words, const Side &offsets)
{
	if (overlap(f.side.p, f.side.extent, words.p, words.extent))
		return fail("bit-planes: the planes and the words overlap");
	if (overlap(f.side.p, f.side.extent, offsets.p, offsets.extent))
		return fail("bit-planes: the planes and the offsets overlap");
	if (overlap(words.p, words.extent, offsets.p, offsets.extent))
		return fail("bit-planes: the words and the offsets overlap");
	return 0;
}

void band_args(const Frames &f, BitplaneArgs *a)
{
	a->batch = f.batch, a->bands = f.bands, a->blocks = f.blocks(), a->cbx = f.cbx, a->cby = f.cby;
	a->pitch = f.pitch, a->bs = f.bs;
	for (int k = 0; k <= f.bands; k++) {
		if (k < f.bands) {
			a->x0[k] = f.table[5 * k], a->y0[k] = f.table[5 * k + 1], a->w[k] = f.table[5 * k + 2], a->h[k] = f.table[5 * k + 3];
			a->blocks_x[k] = a->w[k] > 0 && a->h[k] > 0 ? (a->w[k] + (1 << f.cbx) - 1) >> f.cbx : 0;
		}
		a->first[k] = f.table[5 * k + 4];
	}
}

int zero_offsets(unsigned *offsets, size_t bytes)
{
	if (!bytes)
		return 0;
	if (dwt_hip_is_device_pointer(offsets))
		HIP_TRY(hipMemsetAsync(offsets, 0, bytes, g.stream));
	else
		memset(offsets, 0, bytes);
	return 0;
}

int pack_call(const Frames &f, unsigned long long *words, size_t stream_stride, const Side &words_side, unsigned *offsets, const Side &off_side)
{
	const bool count_only = !words;
	if (f.batch == 0)
		return 0;
	if (check_inited())
		return 1;
	if (f.blocks() == 0) // frames without elements: nothing to launch, their offsets are zeros
		return zero_offsets(offsets, off_side.extent);
	if (grow(g.bp_ws, (size_t)f.batch * f.blocks() * 4))
		return 1;
	char *pp, *op, *wp = (char *)words;
	bool planes_host, off_host, words_host = false;
	if (mirror(f.side, g.bp_planes, true, &pp, &planes_host) || mirror(off_side, g.bp_off, false, &op, &off_host))
		return 1;
	// (a host stream is uploaded first: the words behind a frame's total come back as they were)
	if (!count_only && stream_stride && mirror(words_side, g.bp_words, true, &wp, &words_host))
		return 1;
	BitplaneArgs a{};
	band_args(f, &a);
	a.index = pp;
	a.wide = g.quant_wide != 0 && all16({(uintptr_t)pp, (uintptr_t)f.bs, (uintptr_t)f.pitch});
	a.sizes = (unsigned *)g.bp_ws.p;
	a.offsets = (unsigned *)op;
	a.words = (unsigned long long *)wp, a.stream_stride = stream_stride;
	if (launched(launch_bitplane_sizes(f.index_type, a, g.stream), "bit-plane", "block sizes") ||
	    launched(launch_bitplane_scan(a, g.stream), "bit-plane", "scan"))
		return 1;
	if (!count_only && launched(launch_bitplane_pack(f.index_type, g.bitplane_wave != 0, a, g.stream), "bit-plane", "pack"))
		return 1;
	if (off_host && mirror_back(off_side, g.bp_off))
		return 1;
	if (words_host && mirror_back(words_side, g.bp_words))
		return 1;
	if (off_host || planes_host || words_host)
		HIP_TRY(hipStreamSynchronize(g.stream));
	return 0;
}

} // namespace

} // namespace dwtb

using namespace dwtb;

#pragma GCC visibility push(default)
extern "C" {

int dwt_hip_bitplane_pack_batch(int index_type, const void *index, size_t batch_stride, size_t row_pitch, int batch, int size_x, int size_y,
	int j_max, int cb_log2_x, int cb_log2_y, uint64_t *words, size_t stream_stride, unsigned *offsets)
{
	Frames f;
	if (frames_check(&f, index_type, index, batch_stride, row_pitch, batch, size_x, size_y, j_max, cb_log2_x, cb_log2_y))
		return 1;
	Side off_side, words_side{nullptr, 0, true};
	if (array_check(&off_side, "offsets", offsets, (size_t)f.blocks() + 1, 4, batch) ||
	    (words && array_check(&words_side, "words", words, stream_stride, 8, batch)) || apart(f, words_side, off_side))
		return 1;
	return pack_call(f, (unsigned long long *)words, words ? stream_stride : 0, words_side, offsets, off_side);
}

int dwt_hip_bitplane_unpack_batch(int index_type, const uint64_t *words, size_t stream_stride, const unsigned *offsets, void *index,
	size_t batch_stride, size_t row_pitch, int batch, int size_x, int size_y, int j_max, int cb_log2_x, int cb_log2_y, int drop, int mode)
{
	Frames f;
	if (frames_check(&f, index_type, index, batch_stride, row_pitch, batch, size_x, size_y, j_max, cb_log2_x, cb_log2_y))
		return 1;
	if (drop < 0 || drop > 32)
		return fail("bit-planes: drop %d (0 .. 32)", drop);
	if (mode != DWT_HIP_BITPLANE_KEEP && mode != DWT_HIP_BITPLANE_SHIFT)
		return fail("bit-planes: unknown mode %d", mode);
	Side off_side, words_side;
	if (array_check(&off_side, "offsets", offsets, (size_t)f.blocks() + 1, 4, batch) ||
	    array_check(&words_side, "words", words, stream_stride, 8, batch) || apart(f, words_side, off_side))
		return 1;
	if (f.empty())
		return 0;
	if (check_inited())
		return 1;
	char *pp, *op, *wp = (char *)words;
	bool planes_host, off_host, words_host = false;
	// (host planes with bytes between their elements are uploaded first, so that those come back as they were)
	if (mirror(f.side, g.bp_planes, !f.side.dense, &pp, &planes_host) || mirror(off_side, g.bp_off, true, &op, &off_host))
		return 1;
	if (stream_stride && mirror(words_side, g.bp_words, true, &wp, &words_host))
		return 1;
	BitplaneArgs a{};
	band_args(f, &a);
	a.index = pp;
	a.offsets = (unsigned *)op;
	a.words = (unsigned long long *)wp, a.stream_stride = stream_stride;
	a.drop = drop, a.mode = mode, a.nt = nt_for(f.side.extent);
	a.wide = all16({(uintptr_t)pp, (uintptr_t)f.bs, (uintptr_t)f.pitch}); // (blocks whose rows start on 16-byte boundaries are stored by 16-byte runs)
	if (launched(launch_bitplane_unpack(index_type, g.bitplane_wave != 0, a, g.stream), "bit-plane", "unpack"))
		return 1;
	if (planes_host && mirror_back(f.side, g.bp_planes))
		return 1;
	if (planes_host || off_host || words_host)
		HIP_TRY(hipStreamSynchronize(g.stream));
	return 0;
}

int dwt_hip_bitplane_route(int index_type, const void *index, size_t batch_stride, size_t row_pitch, int batch, int size_x, int size_y,
	int j_max, int cb_log2_x, int cb_log2_y)
{
	Frames f;
	if (frames_check(&f, index_type, index, batch_stride, row_pitch, batch, size_x, size_y, j_max, cb_log2_x, cb_log2_y))
		return -1;
	return g.bitplane_wave != 0 ? 1 : 0;
}

} // extern "C"
#pragma GCC visibility pop
