// dwt_backend_nterm.hip -- the N-term approximation of image groups on the device (keep the coefficients of the N
// largest magnitudes, zero the rest), the magnitude map alone, and their C-ABI (include/libdwt_hip.h).
//
// A call on dense device frames is a memset of the select histograms, one small copy of the ranks, three histogram
// launches and the apply launch (dwt_nterm.hip), whatever the batch, the channel count and N; the thresholds and kept
// counts come back in one copy behind the last launch, and only where the caller asks for them.  Host memory and frames
// whose elements are not adjacent go through the staging path of every other driver (frame_pack_stack /
// frame_unpack_stack: only the frame's own elements are written back).
#include "dwt_backend.h"

#include <climits>

namespace dwtb {

namespace {

// bytes a frame of w x h elements spans: rows sx apart, elements sy (one row: its stride is never used)
long frame_span(long sx, long sy, int w, int h) { return h > 1 ? sx * (long)h : sy * (long)w; }

// what the group entries share: `batch` groups of `channels` frames of w x h, rows sx and elements sy bytes apart
int check_groups(const void *ptr, size_t bstride, int batch, int channels, size_t cstride, long sx, long sy, int w, int h)
{
	if (!ptr)
		return fail("null pointer argument");
	if (channels < 1 || channels > NTERM_MAX_CH)
		return fail("%d channels: a group has 1 to %d", channels, NTERM_MAX_CH);
	if (batch < 0 || w < 0 || h < 0)
		return fail("bad sizes: %d x %d, batch %d", w, h, batch);
	if ((long)w * h > INT_MAX)
		return fail("a frame of %d x %d has more positions than a 32-bit counter holds", w, h);
	if (sy < 4 || (h > 1 && sx < sy * (long)w))
		return fail("bad strides: %ld, %ld bytes", sx, sy);
	if (bstride > (size_t)LONG_MAX / 2 || cstride > (size_t)LONG_MAX / 2)
		return fail("bad strides: batch %zu, channel %zu", bstride, cstride);
	const long span = frame_span(sx, sy, w, h), bs = (long)bstride, cs = (long)cstride;
	if (channels > 1 && cs < span)
		return fail("channels must be apart (channel stride %ld)", cs);
	if (batch > 1 && bs < span)
		return fail("frames must be apart (batch stride %ld)", bs);
	// groups one after the other, or every channel's frames one after the other
	if (channels > 1 && batch > 1 && bs < (channels - 1) * cs + span && cs < (batch - 1) * bs + span)
		return fail("groups and channels overlap (batch stride %ld, channel stride %ld)", bs, cs);
	return 0;
}

// bytes from a group stack's first to behind its last element
long stack_extent(long bs, int batch, int channels, long cs, long span)
{
	return batch < 1 ? 0 : (batch - 1) * bs + (channels - 1) * cs + span;
}

// geometry of the walk
void fill_walk(NtermArgs *a, int batch, int channels, int w, int h)
{
	a->batch = batch;
	a->channels = channels;
	a->w = w;
	a->h = h;
	a->slab_rows = std::max(1, NTERM_SLAB / std::max(w, 1));
	a->slabs = (h + a->slab_rows - 1) / a->slab_rows;
	// 8 workgroups on each of the 256 CUs, shared out over the groups; the rest by the workgroups' slab loop (past the cap: tests/test_hip_grid_limits.py)
	a->bpg = std::max(1, std::min(a->slabs, (2048 + batch - 1) / std::max(batch, 1)));
}

bool all_16(std::initializer_list<const void *> ptrs, std::initializer_list<long> strides)
{
	bool ok = true;
	for (const void *p : ptrs)
		ok = ok && (uintptr_t)p % 16 == 0;
	for (long s : strides)
		ok = ok && s % 16 == 0;
	return ok;
}

// the groups as the kernels take them: where they lie (dense device frames), or packed into frame_a, channel c of
// group b as plane b*channels + c
int stage_groups(void *ptr, long bs, int batch, int channels, long cs, long sx, long sy, int w, int h, bool dev, NtermArgs *a, bool *staged)
{
	if (h == 1)
		sx = sy * w;
	*staged = !(dev && sy == 4);
	if (!*staged) {
		a->img = (char *)ptr;
		a->pitch = sx;
		a->bstride = bs;
		a->cstride = cs;
	} else {
		const long pitch = frame_pitch(4, w);
		if (grow(g.frame_a, (size_t)pitch * h * channels * batch))
			return 1;
		a->img = (char *)g.frame_a.p;
		a->pitch = pitch;
		a->cstride = pitch * h;
		a->bstride = a->cstride * channels;
		for (int b = 0; b < batch; b++)
			if (frame_pack_stack(Frame{(char *)ptr + b * bs, sx, sy, 4, w, h, dev}, channels, cs, a->img + b * a->bstride, pitch))
				return 1;
	}
	a->vec = all_16({a->img}, {a->pitch, a->bstride, a->cstride});
	return 0;
}

int keep_largest(void *ptr, size_t bstride, int batch, int channels, size_t cstride, long sx, long sy, int w, int h, int j_max, int scope,
	const int *keep, float *thr, int *kept)
{
	if (check_inited() || check_groups(ptr, bstride, batch, channels, cstride, sx, sy, w, h))
		return 1;
	if (scope != DWT_HIP_NTERM_FRAME && scope != DWT_HIP_NTERM_DETAILS)
		return fail("unknown scope %d", scope);
	if (!keep)
		return fail("null keep counts");
	if ((thr && dwt_hip_is_device_pointer(thr)) || (kept && dwt_hip_is_device_pointer(kept)))
		return fail("the thresholds and kept counts go to host memory");
	const bool dev = dwt_hip_is_device_pointer(ptr);
	if (dev && check_dev_align({ptr}, {sx, sy, (long)bstride, (long)cstride}))
		return 1;
	NtermArgs a{};
	fill_walk(&a, batch, channels, w, h);
	if (scope == DWT_HIP_NTERM_DETAILS) {
		const int J = dwt_hip_band_levels(w, h, j_max);
		a.lx = (int)(((long)w + (1l << J) - 1) >> J);
		a.ly = (int)(((long)h + (1l << J) - 1) >> J);
	}
	const long M = (long)w * h - (long)a.lx * a.ly;
	if (batch == 0 || M == 0) {
		for (int b = 0; b < batch; b++) {
			if (thr)
				thr[b] = 0.f;
			if (kept)
				kept[b] = 0;
		}
		return 0;
	}
	// workspace: the ranks, the histograms, the records
	const size_t n_rank = ((size_t)batch + 3) & ~(size_t)3, n_hist = (size_t)batch * NTERM_HIST, n_rec = (size_t)batch * NTERM_REC;
	if (grow(g.nterm_ws, (n_rank + n_hist + n_rec) * 4))
		return 1;
	unsigned *ws = (unsigned *)g.nterm_ws.p;
	a.rank = ws;
	a.hist = ws + n_rank;
	a.rec = a.hist + n_hist;
	bool staged;
	if (stage_groups(ptr, (long)bstride, batch, channels, (long)cstride, sx, sy, w, h, dev, &a, &staged))
		return 1;
	static thread_local std::vector<unsigned> host;
	host.resize(std::max((size_t)batch, n_rec));
	for (int b = 0; b < batch; b++)
		host[b] = keep[b] < 1 || keep[b] > M ? (unsigned)M : (unsigned)keep[b]; // vectors.c:281-283
	// (pageable memory: the copy has read it when it returns)
	HIP_TRY(hipMemcpyAsync(ws, host.data(), (size_t)batch * 4, hipMemcpyHostToDevice, g.stream));
	HIP_TRY(hipMemsetAsync(a.hist, 0, n_hist * 4, g.stream));
	// (prof_before counts the launch; under dwt_hip_prof_enable(2) launch p is timed as "level" p, the apply launch as 3)
	for (int pass = 0; pass < 4; pass++) {
		prof_before(pass);
		const hipError_t e = pass < 3 ? launch_nterm_hist(a, pass, g.stream) : launch_nterm_apply(a, g.stream);
		prof_after(pass);
		if (e != hipSuccess)
			return fail("nterm %s launch failed: %s", pass < 3 ? "histogram" : "apply", hipGetErrorString(e));
	}
	if (staged)
		for (int b = 0; b < batch; b++)
			if (frame_unpack_stack(Frame{(char *)ptr + b * (long)bstride, h == 1 ? sy * w : sx, sy, 4, w, h, dev}, channels, (long)cstride,
					a.img + b * a.bstride, a.pitch))
				return 1;
	if (!thr && !kept)
		return 0; // nothing to wait for
	HIP_TRY(hipMemcpyAsync(host.data(), a.rec, n_rec * 4, hipMemcpyDeviceToHost, g.stream));
	HIP_TRY(hipStreamSynchronize(g.stream));
	for (int b = 0; b < batch; b++) {
		if (thr)
			memcpy(&thr[b], &host[(size_t)b * NTERM_REC + 4], 4);
		if (kept)
			kept[b] = (int)host[(size_t)b * NTERM_REC + 5];
	}
	return 0;
}

} // namespace

} // namespace dwtb

using namespace dwtb;

#pragma GCC visibility push(default)
extern "C" {

int dwt_hip_keep_largest_batch(void *ptr, size_t batch_stride, int batch, int channels, size_t channel_stride, int stride_x, int size_x,
	int size_y, int j_max, int scope, const int *keep, float *thr, int *kept)
{
	return keep_largest(ptr, batch_stride, batch, channels, channel_stride, stride_x, 4, size_x, size_y, j_max, scope, keep, thr, kept);
}

int dwt_hip_keep_largest(void *ptr, int stride_x, int stride_y, int size_x, int size_y, int j_max, int scope, int keep, float *thr, int *kept)
{
	return keep_largest(ptr, 0, 1, 1, 0, stride_x, stride_y, size_x, size_y, j_max, scope, &keep, thr, kept);
}

int dwt_hip_magnitude_batch(const void *ptr, size_t batch_stride, int batch, int channels, size_t channel_stride, int stride_x, int size_x,
	int size_y, void *map, size_t map_batch_stride, int map_stride_x)
{
	const int w = size_x, h = size_y;
	if (check_inited() || check_groups(ptr, batch_stride, batch, channels, channel_stride, stride_x, 4, w, h))
		return 1;
	if (!map)
		return fail("null pointer argument");
	if (map_batch_stride > (size_t)LONG_MAX / 2 || (h > 1 && map_stride_x < 4l * w))
		return fail("bad map strides: %d, batch %zu", map_stride_x, map_batch_stride);
	const long span = frame_span(stride_x, 4, w, h), mspan = frame_span(map_stride_x, 4, w, h);
	if (batch > 1 && (long)map_batch_stride < mspan)
		return fail("maps must be apart (map batch stride %zu)", map_batch_stride);
	if (overlap(ptr, (size_t)stack_extent((long)batch_stride, batch, channels, (long)channel_stride, span), map,
			(size_t)stack_extent((long)map_batch_stride, batch, 1, 0, mspan)))
		return fail("the map overlaps the frames");
	const bool dev = dwt_hip_is_device_pointer(ptr);
	if (dev != (bool)dwt_hip_is_device_pointer(map))
		return fail("frames and map lie in one memory space, host or device");
	if (dev && check_dev_align({ptr, map}, {stride_x, (long)batch_stride, (long)channel_stride, map_stride_x, (long)map_batch_stride}))
		return 1;
	if (batch == 0 || w == 0 || h == 0)
		return 0;
	NtermArgs a{};
	fill_walk(&a, batch, channels, w, h);
	bool staged;
	if (stage_groups((void *)ptr, (long)batch_stride, batch, channels, (long)channel_stride, stride_x, 4, w, h, dev, &a, &staged))
		return 1;
	if (!staged) {
		a.map = (char *)map;
		a.map_pitch = h == 1 ? 4l * w : map_stride_x;
		a.map_bstride = (long)map_batch_stride;
	} else {
		a.map_pitch = frame_pitch(4, w);
		a.map_bstride = a.map_pitch * h;
		if (grow(g.frame_b, (size_t)a.map_bstride * batch))
			return 1;
		a.map = (char *)g.frame_b.p;
	}
	a.vec = a.vec && all_16({a.map}, {a.map_pitch, a.map_bstride});
	if (launched(launch_nterm_magnitude(a, g.stream), "nterm", "magnitude"))
		return 1;
	if (staged)
		return frame_unpack_stack(Frame{map, h == 1 ? 4l * w : map_stride_x, 4, 4, w, h, dev}, batch, (long)map_batch_stride, a.map, a.map_pitch);
	return 0;
}

} // extern "C"
#pragma GCC visibility pop
