// dwt_backend_sparse.hip -- sparse coefficient streams: the kept elements of coefficient or index planes packed into
// (position, value) entries in stream order, and scattered back; their C-ABI (include/libdwt_hip.h).
//
// Pack is three launches of dwt_sparse.hip on the context's stream -- the tiles' counts, the scan of one workgroup per
// frame, the entries --, count only the first two, unpack two: the zero fill and the scatter.  The band table in stream
// order and its tiles come from dwt_sparse_geom.c and ride in the kernel arguments; the tiles' counts live in the
// context's workspace.  Each of the three sides -- the planes, the stream, the offsets / counts -- lies in host or in
// device memory on its own; a host side is mirrored like a side of the quantizer (mirror / mirror_back).
#include "dwt_backend.h"

#include <climits>

namespace dwtb {

namespace {

static_assert(SPARSE_TILE_SAMPLES == DWT_HIP_SPARSE_TILE_SAMPLES && SPARSE_GRID_TILES == DWT_HIP_SPARSE_GRID_TILES &&
		SPARSE_GRID_BATCH == DWT_HIP_SPARSE_GRID_BATCH, "the header states the kernels' constants");

int type_of(int type, int *es, unsigned *keep_mask)
{
	switch (type) {
	case DWT_HIP_SPARSE_F32: *es = 4, *keep_mask = 0x7fffffffu; return 0;
	case DWT_HIP_SPARSE_F16: *es = 2, *keep_mask = 0x7fffu; return 0;
	case DWT_HIP_SPARSE_I16: *es = 2, *keep_mask = 0xffffu; return 0;
	case DWT_HIP_SPARSE_I32: *es = 4, *keep_mask = 0xffffffffu; return 0;
	}
	return fail("sparse: unknown element type %d", type);
}

// the frames of a call: `batch` frames of W x H elements of es bytes, and their bands in stream order
struct Frames {
	int batch, W, H, es, bands;
	unsigned keep_mask;
	long pitch, bs; // (a stride that no element is reached by is 0)
	Side side;
	int table[5 * (BAND_MAX_SLOTS + 1)];
	int tiles() const { return table[5 * bands + 4]; }
	bool empty() const { return batch == 0 || W == 0 || H == 0; }
};

int frames_check(Frames *f, int type, const void *p, size_t bs, size_t pitch, int batch, int W, int H, int j_max)
{
	if (type_of(type, &f->es, &f->keep_mask))
		return 1;
	if (batch < 0 || W < 0 || H < 0 || (long)W * H > INT_MAX)
		return fail("sparse: bad sizes (%d frames of %d x %d; a frame holds at most INT_MAX elements)", batch, W, H);
	if (!p)
		return fail("null pointer argument");
	f->batch = batch, f->W = W, f->H = H;
	f->bands = dwt_hip_sparse_bands(W, H, j_max, f->table);
	if (f->bands != 3 * dwt_hip_band_levels(W, H, j_max) + 1)
		return fail("sparse: bad sizes (%d x %d, j_max %d)", W, H, j_max);
	const int es = f->es;
	const size_t lim = (size_t)1 << 46;
	if (bs > lim || pitch > lim)
		return fail("sparse: bad strides of the planes");
	f->bs = batch > 1 ? (long)bs : 0, f->pitch = H > 1 ? (long)pitch : 0;
	if ((uintptr_t)p % es || f->bs % es || f->pitch % es)
		return fail("sparse: the planes' address and strides are multiples of the element size (%d bytes)", es);
	const long row = (long)W * es;
	long one = row;
	if ((H > 1 && f->pitch < row) || !mul_add(&one, std::max(H - 1, 0), f->pitch))
		return fail("sparse: bad row pitch of the planes (%zu bytes for %d elements of %d)", pitch, W, es);
	if (batch > 1 && f->bs < one)
		return fail("sparse: the planes' frames must be apart (batch stride %zu bytes, a frame takes %ld)", bs, one);
	long extent = one;
	if (!mul_add(&extent, std::max(batch - 1, 0), f->bs))
		return fail("sparse: bad strides of the planes");
	f->side = Side{p, f->empty() ? 0 : (size_t)extent, (H < 2 || f->pitch == row) && (batch < 2 || f->bs == one)};
	return 0;
}

bool wide_route(const Frames &f, const void *planes)
{
	return g.sparse_wide != 0 && all16({(uintptr_t)planes, (uintptr_t)f.bs, (uintptr_t)f.pitch});
}

// a dense array of `batch` runs of `stride` words of es bytes (the positions, the values, the offsets)
int array_check(Side *s, const char *what, const void *p, size_t stride, int es, int batch)
{
	if (!p)
		return fail("null pointer argument");
	if ((uintptr_t)p % es)
		return fail("sparse: the address of the %s is a multiple of %d bytes", what, es);
	if (stride > ((size_t)1 << 40))
		return fail("sparse: bad stride of the %s (%zu)", what, stride);
	*s = Side{p, (size_t)batch * stride * es, true};
	return 0;
}

// the regions of a call must not share a byte: the planes with anything, the written arrays with each other
int apart(const Frames &f, std::initializer_list<std::pair<const Side *, const char *>> arrays)
{
	for (auto a = arrays.begin(); a != arrays.end(); ++a) {
		if (overlap(f.side.p, f.side.extent, a->first->p, a->first->extent))
			return fail("sparse: the planes and the %s overlap", a->second);
		for (auto b = a + 1; b != arrays.end(); ++b)
			if (overlap(a->first->p, a->first->extent, b->first->p, b->first->extent))
				return fail("sparse: the %s and the %s overlap", a->second, b->second);
	}
	return 0;
}

void band_args(const Frames &f, SparseArgs *a)
{
	a->batch = f.batch, a->W = f.W, a->H = f.H, a->bands = f.bands, a->tiles = f.tiles();
	a->pitch = f.pitch, a->bs = f.bs, a->keep_mask = f.keep_mask;
	for (int k = 0; k <= f.bands; k++) {
		if (k < f.bands)
			a->x0[k] = f.table[5 * k], a->y0[k] = f.table[5 * k + 1], a->w[k] = f.table[5 * k + 2], a->h[k] = f.table[5 * k + 3];
		a->first[k] = f.table[5 * k + 4];
	}
}

int pack_call(const Frames &f, unsigned *pos, void *val, size_t stream_stride, unsigned *offsets)
{
	const bool count_only = !pos;
	if (f.batch == 0)
		return 0;
	if (check_inited())
		return 1;
	const size_t off_bytes = (size_t)f.batch * (f.bands + 1) * 4;
	char *op;
	bool off_host;
	if (f.tiles() == 0) {
		// frames without elements: nothing to launch, their offsets are zeros
		if (dwt_hip_is_device_pointer(offsets))
			HIP_TRY(hipMemsetAsync(offsets, 0, off_bytes, g.stream));
		else
			memset(offsets, 0, off_bytes);
		return 0;
	}
	// the workspace: the tiles' counts, then the mirror of host offsets
	const size_t tile_bytes = (size_t)align_up((long)((size_t)f.batch * f.tiles() * 4), 256);
	off_host = !dwt_hip_is_device_pointer(offsets);
	if (grow(g.sp_ws, tile_bytes + (off_host ? off_bytes : 0)))
		return 1;
	op = off_host ? (char *)g.sp_ws.p + tile_bytes : (char *)offsets;
	char *pp, *posp = nullptr, *valp = nullptr;
	bool planes_host, pos_host = false, val_host = false;
	if (mirror(f.side, g.sp_planes, true, &pp, &planes_host))
		return 1;
	const Side pos_side{pos, (size_t)f.batch * stream_stride * 4, true}, val_side{val, (size_t)f.batch * stream_stride * f.es, true};
	if (!count_only && stream_stride) {
		// (a host stream is uploaded first: the entries behind a frame's total come back as they were)
		if (mirror(pos_side, g.sp_pos, true, &posp, &pos_host) || mirror(val_side, g.sp_val, true, &valp, &val_host))
			return 1;
	} else if (!count_only) {
		posp = (char *)pos, valp = (char *)val; // (no capacity: nothing is written, nothing is mirrored)
	}
	SparseArgs a{};
	band_args(f, &a);
	a.planes = pp;
	a.wide = wide_route(f, pp);
	a.tile = (unsigned *)g.sp_ws.p;
	a.offsets = (unsigned *)op;
	a.pos = (unsigned *)posp, a.val = valp, a.stream_stride = stream_stride;
	if (launched(launch_sparse_tiles(f.es, false, a, g.stream), "sparse", "tile counts") ||
	    launched(launch_sparse_scan(a, g.stream), "sparse", "scan"))
		return 1;
	if (!count_only && launched(launch_sparse_tiles(f.es, true, a, g.stream), "sparse", "pack"))
		return 1;
	if (off_host)
		HIP_TRY(hipMemcpyAsync(offsets, op, off_bytes, hipMemcpyDeviceToHost, g.stream));
	if (pos_host && mirror_back(pos_side, g.sp_pos))
		return 1;
	if (val_host && mirror_back(val_side, g.sp_val))
		return 1;
	if (off_host || planes_host || pos_host || val_host)
		HIP_TRY(hipStreamSynchronize(g.stream));
	return 0;
}

} // namespace

} // namespace dwtb

using namespace dwtb;

#pragma GCC visibility push(default)
extern "C" {

int dwt_hip_sparse_pack_batch(int type, const void *planes, size_t batch_stride, size_t row_pitch, int batch, int size_x, int size_y,
	int j_max, unsigned *pos, void *val, size_t stream_stride, unsigned *offsets)
{
	Frames f;
	if (frames_check(&f, type, planes, batch_stride, row_pitch, batch, size_x, size_y, j_max))
		return 1;
	if ((pos == nullptr) != (val == nullptr))
		return fail("sparse: positions without values or values without positions (both NULL: count only)");
	Side off_side, pos_side{nullptr, 0, true}, val_side{nullptr, 0, true};
	if (array_check(&off_side, "offsets", offsets, (size_t)f.bands + 1, 4, batch))
		return 1;
	if (pos && (array_check(&pos_side, "positions", pos, stream_stride, 4, batch) || array_check(&val_side, "values", val, stream_stride, f.es, batch)))
		return 1;
	if (apart(f, {{&off_side, "offsets"}, {&pos_side, "positions"}, {&val_side, "values"}}))
		return 1;
	return pack_call(f, pos, val, pos ? stream_stride : 0, offsets);
}

int dwt_hip_sparse_unpack_batch(int type, const unsigned *pos, const void *val, size_t stream_stride, const unsigned *counts,
	size_t counts_stride, void *planes, size_t batch_stride, size_t row_pitch, int batch, int size_x, int size_y)
{
	Frames f;
	if (frames_check(&f, type, planes, batch_stride, row_pitch, batch, size_x, size_y, 0))
		return 1;
	Side pos_side, val_side, cnt_side;
	if (array_check(&pos_side, "positions", pos, stream_stride, 4, batch) || array_check(&val_side, "values", val, stream_stride, f.es, batch) ||
	    array_check(&cnt_side, "counts", counts, counts_stride, 4, batch))
		return 1;
	// (the counts: one word per frame, counts_stride words apart)
	cnt_side.extent = batch ? ((size_t)(batch - 1) * counts_stride + 1) * 4 : 0;
	if (overlap(f.side.p, f.side.extent, pos, pos_side.extent) || overlap(f.side.p, f.side.extent, val, val_side.extent) ||
	    overlap(f.side.p, f.side.extent, counts, cnt_side.extent))
		return fail("sparse: the planes overlap the stream or the counts");
	if (f.empty())
		return 0;
	if (check_inited())
		return 1;
	char *pp, *posp = (char *)pos, *valp = (char *)val;
	bool planes_host, pos_host = false, val_host = false;
	// (host planes with bytes between their elements are uploaded first, so that those come back as they were)
	if (mirror(f.side, g.sp_planes, !f.side.dense, &pp, &planes_host))
		return 1;
	if (stream_stride && (mirror(pos_side, g.sp_pos, true, &posp, &pos_host) || mirror(val_side, g.sp_val, true, &valp, &val_host)))
		return 1;
	// host counts: one word per frame, gathered into the workspace
	const bool cnt_host = !dwt_hip_is_device_pointer(counts);
	SparseUnpackArgs a{};
	a.counts = counts, a.counts_stride = (long)counts_stride;
	if (cnt_host) {
		if (grow(g.sp_ws, (size_t)batch * 4))
			return 1;
		static thread_local std::vector<unsigned> dense; // (pageable memory: the copy has read it when it returns)
		dense.resize(batch);
		for (int b = 0; b < batch; b++)
			dense[b] = counts[(size_t)b * counts_stride];
		HIP_TRY(hipMemcpyAsync(g.sp_ws.p, dense.data(), (size_t)batch * 4, hipMemcpyHostToDevice, g.stream));
		a.counts = (const unsigned *)g.sp_ws.p, a.counts_stride = 1;
	}
	a.planes = pp, a.pitch = f.pitch, a.bs = f.bs, a.batch = batch, a.W = size_x, a.H = size_y;
	a.wide = wide_route(f, pp), a.nt = nt_for(f.side.extent);
	a.pos = (const unsigned *)posp, a.val = valp, a.stream_stride = stream_stride;
	if (launched(launch_sparse_zero(f.es, a, g.stream), "sparse", "zero fill") ||
	    launched(launch_sparse_scatter(f.es, a, g.stream), "sparse", "scatter"))
		return 1;
	if (planes_host && mirror_back(f.side, g.sp_planes))
		return 1;
	if (planes_host || pos_host || val_host || cnt_host)
		HIP_TRY(hipStreamSynchronize(g.stream));
	return 0;
}

int dwt_hip_sparse_route(int type, const void *planes, size_t batch_stride, size_t row_pitch, int batch, int size_x, int size_y)
{
	Frames f;
	if (frames_check(&f, type, planes, batch_stride, row_pitch, batch, size_x, size_y, 0))
		return -1;
	return wide_route(f, planes) ? 1 : 0;
}

} // extern "C"
#pragma GCC visibility pop
