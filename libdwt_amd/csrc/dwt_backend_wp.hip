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
// Pruned trees and the best-basis search of lines: ONE launch of k_wp_tree / k_wp_best (dwt_wp_basis.hip)
// where wp1d takes one launch; otherwise the full tree level by level as above, with small helper kernels after each level
// (costs, the selection, the gathering of the leaves).  Nothing is read back on either route.
// Pruned quadtrees and the best-basis search of images: dense device images run per-level launches only --
// k_wp2d_level with its lift-or-copy switch, a tile cost kernel behind every level of the full tree, one selection launch
// (dwt_wp_basis2d.hip); everything else the staged stack level by level with helper kernels, as for lines.
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
// result lies.  A pass writes its node's samples only, and the nodes of a level tile the line.  `after`: called behind
// every level (the tree routes' helper kernels).
int lines_generic(Wavelet w, bool inverse, Img A, Img B, int n_lines, int N, int levels, Img *res,
	const std::function<int(int, Img)> &after = nullptr)
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
		if (after && after(lev, out)) // (the level just split / rebuilt, and the frame that holds it)
			return 1;
		std::swap(in, out);
	}
	*res = in;
	return 0;
}

// The cross-check route, 2-D: `batch` dense images stacked in A (image b at row b*H), in place through B.  A level: the
// row pass of every node column over all rows of the stack, A -> B, then the column pass of every node row of every
// image, B -> A -- rows before columns both ways, as the float 2-D drivers run their levels.
// `after`: called behind every level with the level just split / rebuilt (the quadtree routes' helper kernels); the frame
// that holds it is A.
int images_generic(Wavelet w, bool inverse, Img A, Img B, int W, int H, int batch, int levels, const std::function<int(int)> &after = nullptr)
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
		if (after && after(lev))
			return 1;
	}
	return 0;
}

// The fused route, 2-D: dense device images, one launch per level.  Level i reads buffer i and writes buffer i + 1;
// buffer 0 is src, the last one dst, the ones between alternate between dst and the scratch frame T.  In place
// (src == dst) an odd number of levels starts from a copy of the images in T.  `tree` (device memory, image b's at tree +
// b*tree_words): every level in the effective quadtrees, a workgroup of a node that is not split copies its tile (s31).
int images_fused(Wavelet w, bool inverse, const char *src, long s_sx, long s_bs, char *dst, long d_sx, long d_bs, int W, int H, int batch,
	int levels, const unsigned *tree = nullptr, long tree_words = 0)
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
		if (tree) {
			Wp2dTreeArgs t{};
			(Wp2dLevelArgs &)t = a;
			t.tree = tree, t.tree_words = tree_words;
			if (launched(launch_wp2d_level_tree(w, inverse, t, g.stream), "packet tree", "2-D level"))
				return 1;
		} else if (launched(launch_wp2d_level(w, inverse, a, g.stream), "packet", "2-D level"))
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


// ---- pruned trees and the best-basis search ------------------------------------------------------------

// what wp1d checks, for the two tree entries; dst may be null where the entry allows it.  *ls: the stride the call runs with
int tree_call_check(const char *what, int wavelet, Wavelet *w, const void *src, const void *dst, long *ls, long es, int n_lines, int N, int levels)
{
	if (wp_wavelet(wavelet, w))
		return 1;
	if (n_lines < 0 || N < 2)
		return fail("%s: bad arguments (%d lines of %d samples; a line has 2 samples or more)", what, n_lines, N);
	const int max_levels = std::min(floor_log2(N), WP_TREE_MAX_LEVELS);
	if (levels < 1 || levels > max_levels)
		return fail("%s: %d levels (a tree over a line of %d samples takes 1 .. %d)", what, levels, N, max_levels);
	if (!src)
		return fail("null pointer argument");
	if (es < 4 || (n_lines > 1 && *ls < 4))
		return fail("%s: bad strides (lines %ld bytes apart, elements %ld)", what, *ls, es);
	if (n_lines <= 1)
		*ls = es * N; // (not used: one line)
	if (*ls < (N - 1l) * es + 4 && (*ls % 4 || *ls * n_lines > es))
		return fail("%s: lines must be apart or interleaved within an element step (line stride %ld, element stride %ld, %d samples)", what,
			*ls, es, N);
	const size_t extent = (size_t)((std::max(n_lines, 1) - 1l) * *ls + (N - 1l) * es + 4);
	if (dst && src != dst && overlap(src, extent, dst, extent))
		return fail("%s: src and dst must be the same lines or not overlap", what);
	return 0;
}

// every pointer of the list that is not null lies where src lies
int same_space(bool dev, std::initializer_list<const void *> ptrs)
{
	for (const void *p : ptrs)
		if (p && dev != (bool)dwt_hip_is_device_pointer(p))
			return fail("src, dst and every table of the call must all be host or all be device pointers");
	return 0;
}

// the scratch of the staged routes, carved from wp_ws: per line two tables of nt doubles, a total, a tree; the frame R
struct TreeWs {
	double *tab, *best, *total;
	unsigned *tree;
	Img R;
};
int tree_ws(int n_lines, int nt, long pitch, TreeWs *ws)
{
	const size_t tab = (size_t)n_lines * nt * 8, tot = (size_t)align_up(n_lines * 8l, 256), tr = (size_t)n_lines * 4 * WP_TREE_WORDS;
	if (grow(g.wp_ws, 2 * tab + tot + tr + (size_t)pitch * n_lines + 256))
		return 1;
	char *p = (char *)g.wp_ws.p;
	ws->tab = (double *)p, p += tab;
	ws->best = (double *)p, p += tab;
	ws->total = (double *)p, p += tot;
	ws->tree = (unsigned *)p, p += align_up((long)tr, 256);
	ws->R = Img{p, pitch, 4};
	return 0;
}

// rows of `width` bytes between two places of one memory space or across PCIe, on the stream
int copy_rows(void *dst, size_t dst_stride, const void *src, size_t src_stride, size_t width, int rows)
{
	HIP_TRY(hipMemcpy2DAsync(dst, dst_stride, src, src_stride, width, (size_t)rows, hipMemcpyDefault, g.stream));
	return 0;
}

// the leaves of the trees out of the frame of one level (mode 0) / the spans of the nodes that are not split back into it (mode 1)
int leaf_copy(Img from, Img to, int n_lines, int N, int levels, const unsigned *tree, long tree_words, int lev, int mode)
{
	return launched(launch_wp_leaf_copy(from.p, to.p, from.sx, n_lines, N, levels, tree, tree_words, lev, mode, g.stream), "packet tree", "leaf copy");
}

// The cross-check route of the transform in given trees (device memory, tree_words apart): the staged frame A, through
// g.frame_b and ws.R.  Forward: the full tree level by level, the leaves of every level gathered in R.  Inverse: every node
// of a level rebuilt, then the source spans of the nodes of that level that are not split put back -- what lies under a
// leaf is rebuilt from garbage and overwritten on the way up.
int tree_generic(Wavelet w, bool inverse, Img A, const TreeWs &ws, int n_lines, int N, int levels, const unsigned *tree, long tree_words, Img *res)
{
	if (grow(g.frame_b, (size_t)A.sx * n_lines))
		return 1;
	const Img B{(char *)g.frame_b.p, A.sx, 4};
	if (!inverse) {
		if (leaf_copy(A, ws.R, n_lines, N, levels, tree, tree_words, 0, 0))
			return 1;
		Img last;
		if (lines_generic(w, false, A, B, n_lines, N, levels, &last,
				[&](int lev, Img out) { return leaf_copy(out, ws.R, n_lines, N, levels, tree, tree_words, lev + 1, 0); }))
			return 1;
		*res = ws.R;
		return 0;
	}
	HIP_TRY(hipMemcpyAsync(ws.R.p, A.p, (size_t)A.sx * n_lines, hipMemcpyDeviceToDevice, g.stream));
	return lines_generic(w, true, A, B, n_lines, N, levels, res,
		[&](int lev, Img out) { return leaf_copy(ws.R, out, n_lines, N, levels, tree, tree_words, lev, 1); });
}

int tree1d(int wavelet, bool inverse, const void *src, void *dst, long ls, long es, int n_lines, int N, int levels, const uint32_t *tree,
	long tree_stride)
{
	Wavelet w;
	if (tree_call_check("packet tree", wavelet, &w, src, dst, &ls, es, n_lines, N, levels))
		return 1;
	if (!dst || !tree)
		return fail("null pointer argument");
	if (tree_stride != 0 && (tree_stride < 4 * WP_TREE_WORDS || tree_stride % 4))
		return fail("packet tree: trees are %d bytes or more apart, a multiple of 4, or 0 for one tree (got %ld)", 4 * WP_TREE_WORDS, tree_stride);
	if (n_lines == 0)
		return 0;
	if (check_inited())
		return 1;
	const bool dev = dwt_hip_is_device_pointer(src);
	if (same_space(dev, {dst, tree}))
		return 1;
	if (dev && check_dev_align({src, dst, tree}, {ls, es}))
		return 1;
	const bool fused = g.wp_fused && N <= N1D_MAX;
	if (dev && fused)
		return launched(launch_wp_tree(w, inverse, src, dst, ls, es, n_lines, N, levels, tree, tree_stride / 4, g.stream), "packet tree", "lines");

	const Frame fs{(void *)src, ls, es, 4, N, n_lines, dev}, fd{dst, ls, es, 4, N, n_lines, dev};
	if (frame_check(fs))
		return 1;
	Img A;
	if (frame_stage(fs, g.frame_a, &A))
		return 1;
	TreeWs ws;
	if (tree_ws(n_lines, 0, fused ? 0 : A.sx, &ws))
		return 1;
	const unsigned *d_tree = tree;
	long d_words = tree_stride / 4;
	if (!dev) { // the trees cross PCIe
		if (copy_rows(ws.tree, 4 * WP_TREE_WORDS, tree, tree_stride ? tree_stride : 4 * WP_TREE_WORDS, 4 * WP_TREE_WORDS, tree_stride ? n_lines : 1))
			return 1;
		d_tree = ws.tree;
		d_words = tree_stride ? WP_TREE_WORDS : 0;
	}
	Img res = A;
	if (fused) {
		if (launched(launch_wp_tree(w, inverse, A.p, A.p, A.sx, 4, n_lines, N, levels, d_tree, d_words, g.stream), "packet tree", "lines"))
			return 1;
	} else if (tree_generic(w, inverse, A, ws, n_lines, N, levels, d_tree, d_words, &res))
		return 1;
	return frame_unpack(fd, res.p, res.sx);
}

int best1d(int wavelet, int kind, float param, const void *src, void *dst, long ls, long es, int n_lines, int N, int levels, uint32_t *tree,
	long tree_stride, double *total, double *node_cost, long cost_stride)
{
	Wavelet w;
	if (tree_call_check("best basis", wavelet, &w, src, dst, &ls, es, n_lines, N, levels))
		return 1;
	if (kind < kWpCostShannon || kind > kWpCostThreshold)
		return fail("best basis: cost %d (DWT_HIP_WP_COST_SHANNON .. _THRESHOLD)", kind);
	if (kind == kWpCostLp && !(param > 0.0f && param < 2.0f))
		return fail("best basis: the l^p cost takes 0 < param < 2 (got %g)", (double)param);
	if (kind == kWpCostThreshold && !(param >= 0.0f && param <= 3.4028234663852886e38f))
		return fail("best basis: the threshold cost takes a finite param >= 0 (got %g)", (double)param);
	if (!dst && !tree && !total && !node_cost)
		return fail("best basis: every output is NULL");
	const int nt = 2 << levels;
	if (tree && (tree_stride < 4 * WP_TREE_WORDS || tree_stride % 4))
		return fail("best basis: trees are %d bytes or more apart, a multiple of 4 (got %ld)", 4 * WP_TREE_WORDS, tree_stride);
	if (node_cost && (cost_stride < 8l * nt || cost_stride % 8))
		return fail("best basis: cost tables of %d levels are %ld bytes or more apart, a multiple of 8 (got %ld)", levels, 8l * nt, cost_stride);
	if (n_lines == 0)
		return 0;
	if (check_inited())
		return 1;
	const bool dev = dwt_hip_is_device_pointer(src);
	if (same_space(dev, {dst, tree, total, node_cost}))
		return 1;
	if (dev && (check_dev_align({src, dst, tree}, {ls, es}) || (uintptr_t)total % 8 || (uintptr_t)node_cost % 8))
		return fail("best basis: device memory takes addresses that are multiples of 4 bytes, of 8 for the doubles");
	const bool fused = g.wp_fused && N <= N1D_MAX;
	WpBestArgs a{};
	a.n_lines = n_lines, a.N = N, a.levels = levels, a.kind = kind, a.param = param;
	if (dev && fused) {
		a.src = (const char *)src, a.dst = (char *)dst, a.line_stride = ls, a.elem_stride = es;
		a.tree = tree, a.tree_words = tree_stride / 4, a.total = total, a.node_cost = node_cost, a.cost_doubles = cost_stride / 8;
		return launched(launch_wp_best(w, a, g.stream), "best basis", "lines");
	}

	// the staging detour: the lines as a dense device frame, dense tables in the scratch, everything spread to the caller's
	const Frame fs{(void *)src, ls, es, 4, N, n_lines, dev}, fd{dst, ls, es, 4, N, n_lines, dev};
	if (frame_check(fs))
		return 1;
	Img A;
	if (frame_stage(fs, g.frame_a, &A))
		return 1;
	TreeWs ws;
	if (tree_ws(n_lines, nt, fused ? 0 : A.sx, &ws))
		return 1;
	Img res = A;
	if (fused) {
		a.src = A.p, a.dst = dst ? A.p : nullptr, a.line_stride = A.sx, a.elem_stride = 4;
		a.tree = ws.tree, a.tree_words = WP_TREE_WORDS, a.total = ws.total, a.node_cost = ws.tab, a.cost_doubles = nt;
		if (launched(launch_wp_best(w, a, g.stream), "best basis", "lines"))
			return 1;
	} else {
		// sweep 1: the full tree, the costs of the nodes of every level behind it
		auto costs = [&](int j, Img f) {
			return launched(launch_wp_cost_level(f.p, f.sx, n_lines, N, j, kind, param, ws.tab, nt, g.stream), "best basis", "level costs");
		};
		if (grow(g.frame_b, (size_t)A.sx * n_lines))
			return 1;
		Img last;
		if (costs(0, A) || lines_generic(w, false, A, Img{(char *)g.frame_b.p, A.sx, 4}, n_lines, N, levels, &last,
				[&](int lev, Img out) { return costs(lev + 1, out); }))
			return 1;
		// the selection works on a copy: the costs stay for the caller, entry 0 takes the total
		HIP_TRY(hipMemcpyAsync(ws.best, ws.tab, (size_t)n_lines * nt * 8, hipMemcpyDeviceToDevice, g.stream));
		if (launched(launch_wp_select(ws.best, n_lines, levels, ws.tree, nullptr, 0, ws.total, ws.tab, nt, g.stream), "best basis", "selection"))
			return 1;
		// sweep 2: the lines again (in place too: dst has not been written yet), the leaves gathered level by level
		if (dst && (frame_stage(fs, g.frame_a, &A) || tree_generic(w, false, A, ws, n_lines, N, levels, ws.tree, WP_TREE_WORDS, &res)))
			return 1;
	}
	if (tree && copy_rows(tree, tree_stride, ws.tree, 4 * WP_TREE_WORDS, 4 * WP_TREE_WORDS, n_lines))
		return 1;
	if (total && copy_rows(total, 8l * n_lines, ws.total, 8l * n_lines, 8l * n_lines, 1))
		return 1;
	if (node_cost && copy_rows(node_cost, cost_stride, ws.tab, 8l * nt, 8l * nt, n_lines))
		return 1;
	if (dst && frame_unpack(fd, res.p, res.sx))
		return 1;
	if (!dev)
		HIP_TRY(hipStreamSynchronize(g.stream));
	return 0;
}


// ---- pruned quadtrees and the best-basis search of image batches ---------------------------------------

// what wp2d checks, for the two quadtree entries; dst may be null where the entry allows it.  *bs: the stride the call runs with
int qtree_call_check(const char *what, int wavelet, Wavelet *w, const void *src, const void *dst, long *bs, int batch, long sx, long sy, int W,
	int H, int levels)
{
	if (wp_wavelet(wavelet, w))
		return 1;
	if (batch < 0 || W < 2 || H < 2)
		return fail("%s: bad arguments (%d images of %d x %d; an image has 2 x 2 samples or more)", what, batch, W, H);
	const int max_levels = std::min(floor_log2(std::min(W, H)), WP_QTREE_MAX_LEVELS);
	if (levels < 1 || levels > max_levels)
		return fail("%s: %d levels (a quadtree over images of %d x %d takes 1 .. %d)", what, levels, W, H, max_levels);
	if (!src)
		return fail("null pointer argument");
	if (sy < 4 || sx < sy * (long)W)
		return fail("%s: bad strides (rows %ld bytes apart, elements %ld; %d samples a row)", what, sx, sy, W);
	const size_t one = (size_t)((H - 1l) * sx + (W - 1l) * sy + 4);
	if (batch > 1 && (size_t)*bs < one)
		return fail("%s: images must be apart (batch stride %ld bytes, an image takes %zu)", what, *bs, one);
	if (batch <= 1)
		*bs = (long)one;
	const size_t extent = (size_t)(std::max(batch, 1) - 1l) * *bs + one;
	if (dst && src != dst && overlap(src, extent, dst, extent))
		return fail("%s: src and dst must be the same images or not overlap", what);
	return 0;
}

// the scratch of the quadtree routes, carved from wp_ws: per image the tile partials, a cost table, a total, a tree; one frame
struct QtreeWs {
	double *part, *tab, *total;
	unsigned *tree;
	char *frame;
};
int qtree_ws(int batch, int levels, long part_doubles, size_t frame_bytes, QtreeWs *ws)
{
	const size_t part = (size_t)align_up(8l * part_doubles * batch, 256), tab = (size_t)align_up(8l * wp_qbase(levels + 1) * batch, 256);
	const size_t tot = (size_t)align_up(8l * batch, 256), tr = (size_t)align_up(4l * WP_QTREE_WORDS * batch, 256);
	if (grow(g.wp_ws, part + tab + tot + tr + frame_bytes + 256))
		return 1;
	char *p = (char *)g.wp_ws.p;
	ws->part = (double *)p, p += part;
	ws->tab = (double *)p, p += tab;
	ws->total = (double *)p, p += tot;
	ws->tree = (unsigned *)p, p += tr;
	ws->frame = p;
	return 0;
}

int qleaf_copy(const char *from, char *to, long pitch, long plane, int W, int H, int batch, int levels, const unsigned *tree, long tree_words,
	int lev, int mode)
{
	return launched(launch_wp_qleaf_copy(from, to, pitch, plane, W, H, batch, levels, tree, tree_words, lev, mode, g.stream), "packet quadtree",
		"leaf copy");
}

// The cross-check route of the transform in given quadtrees (device memory, tree_words apart): the staged stack A, through B
// and R.  Forward: the full tree level by level in A, the leaves of every level gathered in R.  Inverse: every node of a
// level rebuilt in A, then the source rectangles (kept in R) of the nodes of that level that are not split put back -- what
// lies under a leaf is rebuilt from garbage and overwritten on the way up.  *res: where the result lies.
int qtree_generic(Wavelet w, bool inverse, Img A, Img B, char *R, int W, int H, int batch, int levels, const unsigned *tree, long tree_words,
	char **res)
{
	const long plane = A.sx * H;
	if (!inverse) {
		if (qleaf_copy(A.p, R, A.sx, plane, W, H, batch, levels, tree, tree_words, 0, 0))
			return 1;
		if (images_generic(w, false, A, B, W, H, batch, levels,
				[&](int lev) { return qleaf_copy(A.p, R, A.sx, plane, W, H, batch, levels, tree, tree_words, lev + 1, 0); }))
			return 1;
		*res = R;
		return 0;
	}
	HIP_TRY(hipMemcpyAsync(R, A.p, (size_t)plane * batch, hipMemcpyDeviceToDevice, g.stream));
	*res = A.p;
	return images_generic(w, true, A, B, W, H, batch, levels,
		[&](int lev) { return qleaf_copy(R, A.p, A.sx, plane, W, H, batch, levels, tree, tree_words, lev, 1); });
}

int tree2d(int wavelet, bool inverse, const void *src, void *dst, long bs, int batch, long sx, long sy, int W, int H, int levels,
	const uint32_t *tree, long tree_stride)
{
	Wavelet w;
	if (qtree_call_check("packet quadtree", wavelet, &w, src, dst, &bs, batch, sx, sy, W, H, levels))
		return 1;
	if (!dst || !tree)
		return fail("null pointer argument");
	if (tree_stride != 0 && (tree_stride < 4 * WP_QTREE_WORDS || tree_stride % 4))
		return fail("packet quadtree: trees are %d bytes or more apart, a multiple of 4, or 0 for one tree (got %ld)", 4 * WP_QTREE_WORDS,
			tree_stride);
	if (batch == 0)
		return 0;
	if (check_inited())
		return 1;
	const bool dev = dwt_hip_is_device_pointer(src);
	if (same_space(dev, {dst, tree}))
		return 1;
	if (dev && check_dev_align({src, dst, tree}, {bs, sx, sy}))
		return 1;
	if (dev && sy == 4 && images_fused_ok(src, sx, bs, dst, sx, bs, W, H, batch, levels))
		return images_fused(w, inverse, (const char *)src, sx, bs, (char *)dst, sx, bs, W, H, batch, levels, tree, tree_stride / 4);

	const Frame fs{(void *)src, sx, sy, 4, W, H, dev}, fd{dst, sx, sy, 4, W, H, dev};
	if (frame_check(fs))
		return 1;
	if ((long)H * batch > INT_MAX)
		return fail("packet quadtree: too many rows to stage (%ld)", (long)H * batch);
	const long pitch = frame_pitch(4, W), plane = pitch * H;
	QtreeWs ws;
	if (grow(g.frame_a, (size_t)plane * batch) || grow(g.frame_b, (size_t)plane * batch) || qtree_ws(batch, levels, 0, (size_t)plane * batch, &ws))
		return 1;
	if (frame_pack_stack(fs, batch, bs, g.frame_a.p, pitch))
		return 1;
	const unsigned *d_tree = tree;
	long d_words = tree_stride / 4;
	if (!dev) { // the trees cross PCIe
		if (copy_rows(ws.tree, 4 * WP_QTREE_WORDS, tree, tree_stride ? tree_stride : 4 * WP_QTREE_WORDS, 4 * WP_QTREE_WORDS, tree_stride ? batch : 1))
			return 1;
		d_tree = ws.tree;
		d_words = tree_stride ? WP_QTREE_WORDS : 0;
	}
	char *res;
	if (qtree_generic(w, inverse, Img{(char *)g.frame_a.p, pitch, 4}, Img{(char *)g.frame_b.p, pitch, 4}, ws.frame, W, H, batch, levels, d_tree,
			d_words, &res))
		return 1;
	return frame_unpack_stack(fd, batch, bs, res, pitch);
}

int best2d(int wavelet, int kind, float param, const void *src, void *dst, long bs, int batch, long sx, long sy, int W, int H, int levels,
	uint32_t *tree, long tree_stride, double *total, double *node_cost, long cost_stride)
{
	Wavelet w;
	if (qtree_call_check("best basis 2-D", wavelet, &w, src, dst, &bs, batch, sx, sy, W, H, levels))
		return 1;
	if (kind < kWpCostShannon || kind > kWpCostThreshold)
		return fail("best basis 2-D: cost %d (DWT_HIP_WP_COST_SHANNON .. _THRESHOLD)", kind);
	if (kind == kWpCostLp && !(param > 0.0f && param < 2.0f))
		return fail("best basis 2-D: the l^p cost takes 0 < param < 2 (got %g)", (double)param);
	if (kind == kWpCostThreshold && !(param >= 0.0f && param <= 3.4028234663852886e38f))
		return fail("best basis 2-D: the threshold cost takes a finite param >= 0 (got %g)", (double)param);
	if (!dst && !tree && !total && !node_cost)
		return fail("best basis 2-D: every output is NULL");
	const int nq = wp_qbase(levels + 1);
	if (tree && (tree_stride < 4 * WP_QTREE_WORDS || tree_stride % 4))
		return fail("best basis 2-D: trees are %d bytes or more apart, a multiple of 4 (got %ld)", 4 * WP_QTREE_WORDS, tree_stride);
	if (node_cost && (cost_stride < 8l * nq || cost_stride % 8))
		return fail("best basis 2-D: cost tables of %d levels are %ld bytes or more apart, a multiple of 8 (got %ld)", levels, 8l * nq, cost_stride);
	if (batch == 0)
		return 0;
	if (check_inited())
		return 1;
	const bool dev = dwt_hip_is_device_pointer(src);
	if (same_space(dev, {dst, tree, total, node_cost}))
		return 1;
	if (dev && (check_dev_align({src, dst, tree}, {bs, sx, sy}) || (uintptr_t)total % 8 || (uintptr_t)node_cost % 8))
		return fail("best basis 2-D: device memory takes addresses that are multiples of 4 bytes, of 8 for the doubles");
	WpQSelectArgs sel{};
	sel.W = W, sel.H = H, sel.levels = levels, sel.batch = batch;
	QtreeWs ws;

	if (dev && sy == 4 && images_fused_ok(src, sx, bs, dst ? dst : (void *)src, sx, bs, W, H, batch, levels)) {
		// sweep 1: the full tree src -> F0 <-> F1, the tile costs behind the source and behind every level; the selection; sweep
		// 2 (dst given): the pruned transform from src again -- in place too, dst has not been written before that
		const long t_sx = 4l * W, t_bs = t_sx * H;
		long slots = 0;
		for (int j = 0; j <= levels; j++) {
			sel.part_off[j] = slots;
			slots += ((long)wp_tiles(W, j, WP2D_TILE_W) * wp_tiles(H, j, WP2D_TILE_H)) << (2 * j);
		}
		if (grow(g.frame_b, (size_t)t_bs * batch) || qtree_ws(batch, levels, slots, levels > 1 ? (size_t)t_bs * batch : 0, &ws))
			return 1;
		auto costs = [&](int j, const char *f, long f_sx, long f_bs) {
			WpQCostArgs c{f, f_sx, f_bs, W, H, batch, j, kind, param, ws.part + sel.part_off[j], slots};
			return launched(launch_wp_qcost_tiles(c, g.stream), "best basis 2-D", "tile costs");
		};
		if (costs(0, (const char *)src, sx, bs))
			return 1;
		Wp2dLevelArgs a{};
		a.src = (const char *)src, a.src_pitch = sx, a.src_bs = bs;
		a.dst_pitch = t_sx, a.dst_bs = t_bs, a.W = W, a.H = H, a.batch = batch;
		for (int lev = 0; lev < levels; lev++) {
			a.dst = (lev & 1) ? ws.frame : (char *)g.frame_b.p;
			a.level = lev;
			if (launched(launch_wp2d_level(w, false, a, g.stream), "best basis 2-D", "level") || costs(lev + 1, a.dst, t_sx, t_bs))
				return 1;
			a.src = a.dst, a.src_pitch = t_sx, a.src_bs = t_bs;
		}
		sel.part = ws.part, sel.part_stride = slots, sel.tab = ws.tab, sel.tree_ws = ws.tree;
		sel.tree = tree, sel.tree_words = tree_stride / 4, sel.total = total, sel.node_cost = node_cost, sel.cost_doubles = cost_stride / 8;
		if (launched(launch_wp_qselect(sel, g.stream), "best basis 2-D", "selection"))
			return 1;
		return dst ? images_fused(w, false, (const char *)src, sx, bs, (char *)dst, sx, bs, W, H, batch, levels, ws.tree, WP_QTREE_WORDS) : 0;
	}

	// the cross-check route: the batch as a stack of dense device images; device outputs are written where they lie, host
	// outputs cross PCIe from the scratch
	const Frame fs{(void *)src, sx, sy, 4, W, H, dev}, fd{dst, sx, sy, 4, W, H, dev};
	if (frame_check(fs))
		return 1;
	if ((long)H * batch > INT_MAX)
		return fail("best basis 2-D: too many rows to stage (%ld)", (long)H * batch);
	const long pitch = frame_pitch(4, W), plane = pitch * H;
	if (grow(g.frame_a, (size_t)plane * batch) || grow(g.frame_b, (size_t)plane * batch)
		|| qtree_ws(batch, levels, 0, dst ? (size_t)plane * batch : 0, &ws))
		return 1;
	if (frame_pack_stack(fs, batch, bs, g.frame_a.p, pitch))
		return 1;
	const Img A{(char *)g.frame_a.p, pitch, 4}, B{(char *)g.frame_b.p, pitch, 4};
	auto costs = [&](int j) {
		return launched(launch_wp_qcost_level(A.p, pitch, plane, W, H, batch, j, kind, param, ws.tab, nq, g.stream), "best basis 2-D", "level costs");
	};
	if (costs(0) || images_generic(w, false, A, B, W, H, batch, levels, [&](int lev) { return costs(lev + 1); }))
		return 1;
	sel.tab = ws.tab, sel.tree_ws = ws.tree;
	if (dev)
		sel.tree = tree, sel.tree_words = tree_stride / 4, sel.total = total, sel.node_cost = node_cost, sel.cost_doubles = cost_stride / 8;
	else
		sel.total = ws.total;
	if (launched(launch_wp_qselect(sel, g.stream), "best basis 2-D", "selection"))
		return 1;
	if (dst) {
		char *res;
		if (frame_pack_stack(fs, batch, bs, g.frame_a.p, pitch)
			|| qtree_generic(w, false, A, B, ws.frame, W, H, batch, levels, ws.tree, WP_QTREE_WORDS, &res)
			|| frame_unpack_stack(fd, batch, bs, res, pitch))
			return 1;
	}
	if (dev)
		return 0;
	if (tree && copy_rows(tree, tree_stride, ws.tree, 4 * WP_QTREE_WORDS, 4 * WP_QTREE_WORDS, batch))
		return 1;
	if (total && copy_rows(total, 8l * batch, ws.total, 8l * batch, 8l * batch, 1))
		return 1;
	if (node_cost && copy_rows(node_cost, cost_stride, ws.tab, 8l * nq, 8l * nq, batch))
		return 1;
	HIP_TRY(hipStreamSynchronize(g.stream));
	return 0;
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

int dwt_hip_wp_best1d_batch(int wavelet, int cost, float param, const void *src, void *dst, size_t line_stride, size_t elem_stride,
	int n_lines, int N, int levels, uint32_t *tree, size_t tree_stride, double *total, double *node_cost, size_t cost_stride)
{
	if (line_stride > (size_t)LONG_MAX / 2 || elem_stride > INT_MAX || tree_stride > (size_t)LONG_MAX / 2 || cost_stride > (size_t)LONG_MAX / 2)
		return fail("best basis: bad strides");
	return best1d(wavelet, cost, param, src, dst, (long)line_stride, (long)elem_stride, n_lines, N, levels, tree, (long)tree_stride, total,
		node_cost, (long)cost_stride);
}

int dwt_hip_wp_tree1d_batch(int wavelet, int inverse, const void *src, void *dst, size_t line_stride, size_t elem_stride, int n_lines,
	int N, int levels, const uint32_t *tree, size_t tree_stride)
{
	if (line_stride > (size_t)LONG_MAX / 2 || elem_stride > INT_MAX || tree_stride > (size_t)LONG_MAX / 2)
		return fail("packet tree: bad strides");
	return tree1d(wavelet, inverse != 0, src, dst, (long)line_stride, (long)elem_stride, n_lines, N, levels, tree, (long)tree_stride);
}

int dwt_hip_wp_best2d_batch(int wavelet, int cost, float param, const void *src, void *dst, size_t batch_stride, int batch, int stride_x,
	int stride_y, int size_x, int size_y, int levels, uint32_t *tree, size_t tree_stride, double *total, double *node_cost, size_t cost_stride)
{
	if (batch_stride > (size_t)LONG_MAX / 2 || stride_x < 0 || stride_y < 0 || tree_stride > (size_t)LONG_MAX / 2 || cost_stride > (size_t)LONG_MAX / 2)
		return fail("best basis 2-D: bad strides");
	return best2d(wavelet, cost, param, src, dst, (long)batch_stride, batch, stride_x, stride_y, size_x, size_y, levels, tree, (long)tree_stride,
		total, node_cost, (long)cost_stride);
}

int dwt_hip_wp_tree2d_batch(int wavelet, int inverse, const void *src, void *dst, size_t batch_stride, int batch, int stride_x, int stride_y,
	int size_x, int size_y, int levels, const uint32_t *tree, size_t tree_stride)
{
	if (batch_stride > (size_t)LONG_MAX / 2 || stride_x < 0 || stride_y < 0 || tree_stride > (size_t)LONG_MAX / 2)
		return fail("packet quadtree: bad strides");
	return tree2d(wavelet, inverse != 0, src, dst, (long)batch_stride, batch, stride_x, stride_y, size_x, size_y, levels, tree, (long)tree_stride);
}

} // extern "C"
#pragma GCC visibility pop
