// dwt_backend_wp.hip -- the wavelet packet transforms of row and image batches on the device, and their C-ABI
// (include/libdwt_hip.h).
//
// Every node of every level is split again; node geometry is wp_node (dwt_kernels.h).  Routes:
//   1-D, lines of up to N1D_MAX samples: every level in ONE launch of k_wp_lines (dwt_wp1d.hip), straight from src to dst
//        for device lines, in the staged frame for host memory;
//   2-D, dense device images: ONE launch of k_wp2d_level (dwt_wp2d.hip) per level for the whole batch, out of place
//        src -> dst <-> one scratch frame, arranged so that the last level lands in dst;
//   everything else -- longer lines, strided image elements, and every call under option "wp_fused" = 0 -- level by level in
//        two dense staged frames, each node through the exact line passes (launch_line_pass).  Same bits.
#include "dwt_backend.h"

#include <climits>

namespace dwtb {

namespace {

int wp_wavelet(int wavelet, Wavelet *w)
{
	if (!wavelet_of(wavelet, w) || (*w != kCdf97S && *w != kCdf53S && *w != kInterp53S))
		return fail("wavelet packets take DWT_HIP_CDF97_S, DWT_HIP_CDF53_S or DWT_HIP_INTERP53_S (got wavelet %d)", wavelet);
	return 0;
}

int floor_log2(int x)
{
	int n = 0;
	while (n < 30 && (2 << n) <= x)
		n++;
	return n;
}

int line_pass(Wavelet w, bool inverse, const char *in, char *out, long ls, long es, int n_lines, int N, bool along_lines)
{
	// (the slow axis of the pass's grid -- the lines, or along_lines the pairs of a line -- takes 65535 blocks)
	if (along_lines && (N + 1) / 2 > 65535)
		return fail("packets: a column of %d samples is too long for the line passes", N);
	const int chunk = along_lines ? n_lines : 65535;
	for (int l0 = 0; l0 < n_lines; l0 += chunk)
		if (launched(launch_line_pass(w, inverse, in + l0 * ls, out + l0 * ls, ls, es, std::min(chunk, n_lines - l0), N, (N + 1) >> 1, along_lines,
				g.stream), "packet", "line pass"))
			return 1;
	return 0;
}

// The cross-check route, 1-D: the dense frame A (n_lines rows of N samples) level by level, A <-> B; *res: where the
// result lies.  A pass writes its node's samples only, and the nodes of a level tile the line.
int lines_generic(Wavelet w, bool inverse, Img A, Img B, int n_lines, int N, int levels, Img *res)
{
	Img in = A, out = B;
	for (int step = 0; step < levels; step++) {
		const int lev = inverse ? levels - 1 - step : step;
		for (int q = 0; q < (1 << lev); q++) {
			int s, n;
			wp_node(N, lev, q, &s, &n);
			if (line_pass(w, inverse, in.p + 4l * s, out.p + 4l * s, in.sx, 4, n_lines, n, false))
				return 1;
		}
		std::swap(in, out);
	}
	*res = in;
	return 0;
}

// The cross-check route, 2-D: `batch` dense images stacked in A (image b at row b*H), in place through B.  A level: the
// row pass of every node column over all rows of the stack, A -> B, then the column pass of every node row of every
// image, B -> A -- rows before columns both ways, as the float 2-D drivers run their levels.
int images_generic(Wavelet w, bool inverse, Img A, Img B, int W, int H, int batch, int levels)
{
	for (int step = 0; step < levels; step++) {
		const int lev = inverse ? levels - 1 - step : step;
		for (int q = 0; q < (1 << lev); q++) {
			int s, n;
			wp_node(W, lev, q, &s, &n);
			if (line_pass(w, inverse, A.p + 4l * s, B.p + 4l * s, A.sx, 4, H * batch, n, false))
				return 1;
		}
		for (int b = 0; b < batch; b++)
			for (int q = 0; q < (1 << lev); q++) {
				int s, n;
				wp_node(H, lev, q, &s, &n);
				const long off = ((long)b * H + s) * A.sx;
				if (line_pass(w, inverse, B.p + off, A.p + off, 4, A.sx, W, n, true))
					return 1;
			}
	}
	return 0;
}

// The fused route, 2-D: dense device images, one launch per level.  Level i reads buffer i and writes buffer i + 1;
// buffer 0 is src, the last one dst, the ones between alternate between dst and the scratch frame T.  In place
// (src == dst) an odd number of levels starts from a copy of the images in T.
int images_fused(Wavelet w, bool inverse, const char *src, long s_sx, long s_bs, char *dst, long d_sx, long d_bs, int W, int H, int batch,
	int levels)
{
	const long t_sx = 4l * W, t_bs = t_sx * H;
	const bool in_place = src == dst;
	if ((levels > 1 || in_place) && grow(g.frame_b, (size_t)t_bs * batch))
		return 1;
	char *const T = (char *)g.frame_b.p;
	const char *in = src;
	long in_sx = s_sx, in_bs = s_bs;
	if (in_place && (levels & 1)) {
		for (int b = 0; b < batch; b++)
			if (copy_rect(Img{T + b * t_bs, t_sx, 4}, 0, 0, Img{dst + b * d_bs, d_sx, 4}, 0, 0, W, H))
				return 1;
		in = T, in_sx = t_sx, in_bs = t_bs;
	}
	for (int step = 0; step < levels; step++) {
		const bool to_dst = ((levels - 1 - step) & 1) == 0;
		Wp2dLevelArgs a{};
		a.src = in, a.src_pitch = in_sx, a.src_bs = in_bs;
		a.dst = to_dst ? dst : T, a.dst_pitch = to_dst ? d_sx : t_sx, a.dst_bs = to_dst ? d_bs : t_bs;
		a.W = W, a.H = H, a.batch = batch;
		a.level = inverse ? levels - 1 - step : step;
		if (launched(launch_wp2d_level(w, inverse, a, g.stream), "packet", "2-D level"))
			return 1;
		in = a.dst, in_sx = a.dst_pitch, in_bs = a.dst_bs;
	}
	return 0;
}

bool images_fused_ok(const void *src, long s_sx, long s_bs, void *dst, long d_sx, long d_bs, int W, int H, int batch, int levels)
{
	if (!g.wp_fused)
		return false;
	for (int lev = 0; lev < levels; lev++)
		if (!wp2d_level_fits(Wp2dLevelArgs{(const char *)src, s_sx, s_bs, (char *)dst, d_sx, d_bs, W, H, batch, lev}))
			return false;
	return true;
}

int wp1d(int wavelet, bool inverse, const void *src, void *dst, long ls, long es, int n_lines, int N, int levels)
{
	Wavelet w;
	if (wp_wavelet(wavelet, &w))
		return 1;
	if (n_lines < 0 || N < 2)
		return fail("packets 1-D: bad arguments (%d lines of %d samples; a line has 2 samples or more)", n_lines, N);
	if (levels < 1 || levels > floor_log2(N))
		return fail("packets 1-D: %d levels (a line of %d samples takes 1 .. %d)", levels, N, floor_log2(N));
	if (!src || !dst)
		return fail("null pointer argument");
	if (es < 4 || (n_lines > 1 && ls < 4))
		return fail("packets 1-D: bad strides (lines %ld bytes apart, elements %ld)", ls, es);
	if (n_lines == 0)
		return 0;
	if (n_lines == 1)
		ls = es * N; // (not used: one line)
	// no sample of a line may be a sample of another line: the lines lie apart, or interleaved -- all of them inside one
	// element step (line y the channel y of n_lines or more)
	if (ls < (N - 1l) * es + 4 && (ls % 4 || ls * n_lines > es))
		return fail("packets 1-D: lines must be apart or interleaved within an element step (line stride %ld, element stride %ld, %d samples)",
			ls, es, N);
	const size_t extent = (size_t)((n_lines - 1l) * ls + (N - 1l) * es + 4);
	if (src != dst && overlap(src, extent, dst, extent))
		return fail("packets 1-D: src and dst must be the same lines or not overlap");
	if (check_inited())
		return 1;
	const bool dev = dwt_hip_is_device_pointer(dst);
	if (dev != (bool)dwt_hip_is_device_pointer(src))
		return fail("src and dst must both be host or both be device pointers");
	if (dev && check_dev_align({src, dst}, {ls, es}))
		return 1;
	const bool fused = g.wp_fused && N <= N1D_MAX;
	if (dev && fused)
		return launched(launch_wp_lines(w, inverse, src, dst, ls, es, n_lines, N, levels, g.stream), "packet", "lines");

	// the staging detour: the lines as a dense device frame, transformed there, spread to dst
	const Frame fs{(void *)src, ls, es, 4, N, n_lines, dev}, fd{dst, ls, es, 4, N, n_lines, dev};
	if (frame_check(fs))
		return 1;
	Img A;
	if (frame_stage(fs, g.frame_a, &A))
		return 1;
	Img res = A;
	if (fused) {
		if (launched(launch_wp_lines(w, inverse, A.p, A.p, A.sx, 4, n_lines, N, levels, g.stream), "packet", "lines"))
			return 1;
	} else {
		if (grow(g.frame_b, (size_t)A.sx * n_lines))
			return 1;
		if (lines_generic(w, inverse, A, Img{(char *)g.frame_b.p, A.sx, 4}, n_lines, N, levels, &res))
			return 1;
	}
	return frame_unpack(fd, res.p, res.sx);
}

int wp2d(int wavelet, bool inverse, const void *src, void *dst, long bs, int batch, long sx, long sy, int W, int H, int levels)
{
	Wavelet w;
	if (wp_wavelet(wavelet, &w))
		return 1;
	if (batch < 0 || W < 2 || H < 2)
		return fail("packets 2-D: bad arguments (%d images of %d x %d; an image has 2 x 2 samples or more)", batch, W, H);
	const int max_levels = std::min(floor_log2(std::min(W, H)), WP2D_MAX_LEVELS);
	if (levels < 1 || levels > max_levels)
		return fail("packets 2-D: %d levels (images of %d x %d take 1 .. %d)", levels, W, H, max_levels);
	if (!src || !dst)
		return fail("null pointer argument");
	if (sy < 4 || sx < sy * (long)W)
		return fail("packets 2-D: bad strides (rows %ld bytes apart, elements %ld; %d samples a row)", sx, sy, W);
	const size_t one = (size_t)((H - 1l) * sx + (W - 1l) * sy + 4);
	if (batch > 1 && (size_t)bs < one)
		return fail("packets 2-D: images must be apart (batch stride %ld bytes, an image takes %zu)", bs, one);
	if (batch == 0)
		return 0;
	if (batch == 1)
		bs = (long)one;
	const size_t extent = (size_t)(batch - 1l) * bs + one;
	if (src != dst && overlap(src, extent, dst, extent))
		return fail("packets 2-D: src and dst must be the same images or not overlap");
	if (check_inited())
		return 1;
	const bool dev = dwt_hip_is_device_pointer(dst);
	if (dev != (bool)dwt_hip_is_device_pointer(src))
		return fail("src and dst must both be host or both be device pointers");
	if (dev && check_dev_align({src, dst}, {bs, sx, sy}))
		return 1;
	if (dev && sy == 4 && images_fused_ok(src, sx, bs, dst, sx, bs, W, H, batch, levels))
		return images_fused(w, inverse, (const char *)src, sx, bs, (char *)dst, sx, bs, W, H, batch, levels);

	// the staging detour: the batch as a stack of dense device images, transformed in place there, spread to dst
	const Frame fs{(void *)src, sx, sy, 4, W, H, dev}, fd{dst, sx, sy, 4, W, H, dev};
	if (frame_check(fs))
		return 1;
	if ((long)H * batch > INT_MAX)
		return fail("packets 2-D: too many rows to stage (%ld)", (long)H * batch);
	const long pitch = frame_pitch(4, W), plane = pitch * H;
	if (grow(g.frame_a, (size_t)plane * batch) || frame_pack_stack(fs, batch, bs, g.frame_a.p, pitch))
		return 1;
	char *const A = (char *)g.frame_a.p;
	if (images_fused_ok(A, pitch, plane, A, pitch, plane, W, H, batch, levels)) {
		if (images_fused(w, inverse, A, pitch, plane, A, pitch, plane, W, H, batch, levels))
			return 1;
	} else {
		if (grow(g.frame_b, (size_t)plane * batch))
			return 1;
		if (images_generic(w, inverse, Img{A, pitch, 4}, Img{(char *)g.frame_b.p, pitch, 4}, W, H, batch, levels))
			return 1;
	}
	return frame_unpack_stack(fd, batch, bs, A, pitch);
}

} // namespace

} // namespace dwtb

using namespace dwtb;

#pragma GCC visibility push(default)
extern "C" {

int dwt_hip_wp_nodes(int N, int level, int *start, int *len)
{
	if (N < 1 || level < 0 || level > floor_log2(N))
		return -1;
	for (int k = 0; k < (1 << level); k++) {
		int s, n;
		wp_node(N, level, k, &s, &n);
		if (start)
			start[k] = s;
		if (len)
			len[k] = n;
	}
	return 1 << level;
}

int dwt_hip_wp_freq_order(int level, int *perm)
{
	if (level < 0 || level > 30)
		return -1;
	for (int f = 0; perm && f < (1 << level); f++)
		perm[f] = f ^ (f >> 1);
	return 1 << level;
}

int dwt_hip_wp1d_batch(int wavelet, int inverse, const void *src, void *dst, size_t line_stride, size_t elem_stride, int n_lines, int N,
	int levels)
{
	if (line_stride > (size_t)LONG_MAX / 2 || elem_stride > INT_MAX)
		return fail("packets 1-D: bad strides");
	return wp1d(wavelet, inverse != 0, src, dst, (long)line_stride, (long)elem_stride, n_lines, N, levels);
}

int dwt_hip_wp2d_batch(int wavelet, int inverse, const void *src, void *dst, size_t batch_stride, int batch, int stride_x, int stride_y,
	int size_x, int size_y, int levels)
{
	if (batch_stride > (size_t)LONG_MAX / 2 || stride_x < 0 || stride_y < 0)
		return fail("packets 2-D: bad strides");
	return wp2d(wavelet, inverse != 0, src, dst, (long)batch_stride, batch, stride_x, stride_y, size_x, size_y, levels);
}

} // extern "C"
#pragma GCC visibility pop
