// dwt_kernels.h -- launch interface between the backend (dwt_backend.hip) and the
// HIP kernels (dwt_sweep2d.hip, dwt_vol3d.hip, dwt_interleaved.hip).  Internal to the shared library.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace dwt {

enum Wavelet { kCdf97S = 0, kCdf53I = 1, kCdf53S = 2, kCdf97D = 3, kCdf53D = 4, kCdf97I = 5,
	kCdf97SFma = 6 /* internal: float 9/7 with contracted steps, option "fma" */,
	kCdf53SNew = 7 /* internal: float 5/3 of dwt-simple.c (odd scale 1/zeta in float), interleaved layout only */,
	kCdf97IIp = 8 /* internal: fixed-point int 9/7 of the interleaved in-place drivers (rounded terms added) */,
	kInterp53S = 9 /* interpolating 5/3 float (public id DWT_HIP_INTERP53_S = 6): predict step only */,
	kCdf53I16 = 10 /* reversible int16 5/3 in JPEG 2000 order (public id DWT_HIP_CDF53_I16 = 8): columns before rows */,
	kCdf97H = 11 /* float 9/7 on binary16 storage (public id DWT_HIP_CDF97_H = 9): binary32 arithmetic, one rounding per level */ };
constexpr int kWavelets = kCdf97H + 1; // one past the LAST enumerator: a new one moves this, and the table below then wants its row

// What the drivers branch on per wavelet, one row per enumerator in its order.  id: the public one (enum dwt_hip_wavelet),
// -1 internal only.  cols_fwd / cols_inv: a level's exact column pass comes before its row pass.  lone: a line of one sample
// is passed through untouched (the int kernels, src/libdwt.c:10961).  skip1: a direction that has one line is skipped (only
// the 9/7 drivers guard on lines > 1).  line_as: the wavelet the exact line passes run as -- another one: on a binary32 copy
// of the level's frame, widened before the passes and narrowed after them.
struct WaveletFacts {
	int es, id;
	bool cols_fwd, cols_inv, lone, skip1;
	Wavelet line_as;
};
constexpr WaveletFacts kWaveletFacts[] = {
	{4, 0, false, false, false, true, kCdf97S},
	{4, 1, false, true, true, false, kCdf53I}, // (the int32 inverses undo columns first)
	{4, 2, false, false, false, false, kCdf53S},
	{8, 3, false, false, false, false, kCdf97D},
	{8, 4, false, false, false, false, kCdf53D},
	{4, 5, false, true, true, false, kCdf97I},
	{4, -1, false, false, false, false, kCdf97SFma},
	{4, -1, false, false, false, false, kCdf53SNew},
	{4, -1, false, false, false, false, kCdf97IIp},
	{4, 6, false, false, false, false, kInterp53S},
	{2, 8, true, false, true, false, kCdf53I16}, // (2D_SD: columns before rows forward, the mirror inverse)
	{2, 9, false, false, false, true, kCdf97S},
};
static_assert(sizeof(kWaveletFacts) / sizeof(kWaveletFacts[0]) == kWavelets, "a row of kWaveletFacts for every enumerator of Wavelet");
constexpr const WaveletFacts &facts(Wavelet w) { return kWaveletFacts[w]; }
inline int elem_size(Wavelet w) { return facts(w).es; }
constexpr bool widened(Wavelet w) { return facts(w).line_as != w; }

// Tuning knobs of the fused sweep kernels (set through dwt_hip_set_option).
struct SweepTuning {
	int cpt = 0;        // columns per lane: 4 or 8; 0 = choose from the level width
	int tile_pairs = 0; // output row pairs per wave tile; 0 = choose from the level height
	int waves = 4;      // waves per workgroup (each wave owns one tile)
	int xcd_swizzle = 1; // remap workgroups so neighbouring tiles share an XCD's L2
	int ring = 0;        // LDS ring rows per wave (8 or 16); 0 = auto
	int nt = 7;          // forward cache policy: loads and detail stores are non-temporal; bit 2 keeps the LL band's
	                     // stores temporal (the next level reads it), bit 3 takes the neighbour taps by wavefront shifts
	int nt_auto = 1;     // forward: drop bit 2 of `nt` when the launch's LL bands exceed the Infinity Cache
	int ring_inv = 8;    // inverse sweep ring rows (8 or 16)
	int inv_pairs = 0;   // inverse: tile height (row pairs) of the large levels under the launcher's rule; 0 = 16 (32 for the levels of an in-place call)
	int inv_ll_temporal = 1; // inverse: a level that is not the last stores its result temporal when it fits the Infinity Cache
	int fuse01_ring = 0; // the fused pair of levels 0 and 1 (launch_fwd01): its ring rows per wave, 16 or 8; 0 = the launcher's rule.
	                     // Its own knob: `ring` = 8 keeps a call level by level
	int fuse01_updown = -1; // the fused pair: which tile rows march upward -- 0 none, 1 the odd ones, 2 the even ones; -1 = the launcher's rule
};

// In-place level of the interleaved layout (input image == output image): a snapshot of what a tile reads of its
// NEIGHBOURS' samples, taken before the level's launch (launch_il_shell).  A tile's own samples are still unwritten
// when it reads them (its stores trail its loads); everything else it reads comes from here.  Tiles of 256 columns x
// `tile_pairs` row pairs.
struct IlShell {
	const float *rows = nullptr;  // 9 rows around every boundary between tile rows: boundary k (rows 2 k tile_pairs - 5 .. + 3)
	long rows_pitch = 0;          //   at slot 9 (k - 1) + i; whole rows
	const float *cols = nullptr;  // per image row the 8 columns around every boundary between tile columns: boundary b
	long cols_pitch = 0;          //   (columns 256 (b + 1) - 4 .. + 3) at 8 b
	const float *top = nullptr;   // rows 0 .. 13, whole (input of the top border strip)
	long top_pitch = 0;
	const float *right = nullptr; // columns right_x0 .. W - 1 of every row (input of the right border strip)
	long right_pitch = 0;
	int right_x0 = 0;
	int tile_pairs = 0;
};
constexpr int kIlShellRight = 20; // floats per row of IlShell::right
// bytes of scratch a shell of a W x H level takes; 0 = this shape cannot run in place (narrow last tile column, short tiles)
size_t il_shell_bytes(int W, int H, int tile_pairs);
// fills the shell from the image (pitch in elements) into `scratch` (il_shell_bytes) and returns its description
hipError_t launch_il_shell(const float *img, long pitch, int W, int H, int tile_pairs, float *scratch, IlShell *sh, hipStream_t s);
// the tile height launch_fwd_level / launch_inv_level give an interleaved single-image level under these settings
int il_sweep_tile_pairs(const SweepTuning &t, int W, int H, bool inverse);
// whether launch_fwd_level / launch_inv_level take a kernel that can carry a copy along (FwdLevelArgs::ride) for this Mallat level
bool sweep_ride_ok(const SweepTuning &t, int W, int H, int batch, bool inverse);

// One decomposition level, forward, dense frame (size_o == size_i, W,H >= 2).
// Reads the W x H region at `in`; writes LL (ceil(W/2) x ceil(H/2)) to `out_ll` and
// the three detail subbands at their Mallat offsets relative to `out_h`:
// HL at (0, Wd), LH at (Hd, 0), HH at (Hd, Wd), Wd = ceil(W/2), Hd = ceil(H/2).
// Pitches are in ELEMENTS.  `batch` images lie `*_bstride` elements apart.
struct CopyRects;
struct FwdLevelArgs {
	const void *in;
	long in_pitch, in_bstride;
	void *out_ll;
	long ll_pitch, ll_bstride;
	void *out_h;
	long h_pitch, h_bstride;
	int W, H, batch;
	int interleaved = 0; // 1: write rows/columns interleaved to out_h (3-D path / in-place lifting layout)
	int plain_ends = 0;  // 1: line ends as reflection gives them, c*(x+x), not the reference's end form (dwt_lift.h): the 3-D
	                     // path's xy sweep, which must give the bits of the fused 3-D level kernels (they keep the reflected form)
	int il_ll = 0;       // interleaved only: also write the LL samples densely to out_ll
	int temporal = 0;    // 1: every store temporal (the outputs are read again at once: staging of an in-place call)
	int pair_lo = 0, pair_hi = 0; // pair_hi > 0: only the tiles that start at a row pair in [pair_lo, pair_hi) -- multiples of 64 --
	                              // run (a level computed band by band while its input is still arriving over PCIe)
	IlShell sh;          // interleaved only, in place (in == out_h, out_step 1): the neighbours' samples come from this snapshot
	// Mallat layout, one image: copy blocks [ride_lo, ride_hi) of a rectangle copy that does not depend on this level run
	// as extra workgroups BEHIND the level's tiles in the same launch (the staged subbands of an in-place call going back
	// while the small, latency-bound levels run: launch_copy_rects_plan)
	const CopyRects *ride = nullptr;
	int ride_lo = 0, ride_hi = 0;
	int unused = 0;      // free: keeps out_step at its offset (moving it changes the compiled kernels); the next new field can take it
	int out_step = 1;    // interleaved only: elements between neighbouring samples of an output row -- 2^j when the level
	                     // is written straight to the lattice it lives on in a larger image (h_pitch: that lattice's row
	                     // pitch); with il_ll the samples at (even row, even column) are then left to the deeper levels
};

// One reconstruction level, inverse, dense frame.  Reads LL from `in_ll` and the
// detail subbands at their Mallat offsets relative to `in_h`; writes the W x H
// interleaved result to `out`.
struct InvLevelArgs {
	const void *in_ll;
	long ll_pitch, ll_bstride;
	const void *in_h;
	long h_pitch, h_bstride;
	void *out;
	long out_pitch, out_bstride;
	int W, H, batch;
	int interleaved = 0; // 1: interleaved input: even rows at in_ll (row r/2), odd rows at in_h (row r/2)
	int plain_ends = 0;  // see FwdLevelArgs
	int temporal_out = 0; // Mallat: the result is the next level's low-pass input and fits the Infinity Cache: stored temporal
	int pair_lo = 0, pair_hi = 0; // pair_hi > 0: only the tiles that start at a row pair in [pair_lo, pair_hi) run (see FwdLevelArgs)
	const CopyRects *ride = nullptr; // see FwdLevelArgs
	int ride_lo = 0, ride_hi = 0;
	// interleaved only -- a level read straight from the lattice it lives on in a larger image:
	IlShell sh;                   // in place (in_ll == out, in_step 1): the neighbours' samples come from this snapshot
	int in_step = 1;              // elements between neighbouring samples of a source row (2^j on the lattice of level j)
	const void *in_ll2 = nullptr; // dense low-pass band (ceil(W/2) x ceil(H/2), the level below's result): replaces the
	long ll2_pitch = 0;           // samples at (even row, even column) of the source
};

// `strip` (interleaved layout, float 9/7 both ways and fdwt2_cdf53 forward, one image of 64 samples or more either
// way): the launch also computes the level's border strips in the reference's phase order and its tiles leave those
// samples alone (dwt_il_strip.h)
struct IlStripArgs;
hipError_t launch_fwd_level(Wavelet w, const FwdLevelArgs &a, const SweepTuning &t, hipStream_t s, const IlStripArgs *strip = nullptr);

// Levels 0 AND 1 of a forward float 9/7 transform (Mallat, out of place) in ONE sweep over the level-0 sweep's own tiles,
// 512 columns apart, each wave computing the 8 LL columns beyond its seams again for itself (k_fwd_sweep01): `a`
// describes level 0, except that out_ll / ll_pitch / ll_bstride are LEVEL 1's LL band -- level 0's is
// never written -- and level 1's detail subbands go to their Mallat places relative to out_h as well.  Same bits as the
// two launches.  fwd01_can: W and H multiples of 4, both levels of 64 x 64 or more; fwd01_tiles: tiles per row.
bool fwd01_can(Wavelet w, int W, int H);
int fwd01_tiles(int W);
bool fwd01_has_ring(int ring); // SweepTuning::fuse01_ring: a depth the sweep has a kernel for
bool fwd01_has_updown(int v);  // SweepTuning::fuse01_updown: -1, 0, 1 or 2
int fwd01_updown(const SweepTuning &t, int W, int H, int batch); // the tile rows that march upward in launch_fwd01's launch (0, 1, 2)
hipError_t launch_fwd01(const FwdLevelArgs &a, const SweepTuning &t, hipStream_t s);

hipError_t launch_inv_level(Wavelet w, const InvLevelArgs &a, const SweepTuning &t, hipStream_t s, const IlStripArgs *strip = nullptr);
// the same two sweeps for the double-precision wavelets (dwt_sweep2d_d.hip); pitches in 8-byte ELEMENTS
hipError_t launch_fwd_level_d(Wavelet w, const FwdLevelArgs &a, const SweepTuning &t, hipStream_t s);
hipError_t launch_inv_level_d(Wavelet w, const InvLevelArgs &a, const SweepTuning &t, hipStream_t s);
// the two sweeps of the int16 5/3 (dwt_sweep2d_i16.hip): pitches in 2-byte ELEMENTS; the images' bases and pitches are
// multiples of 4 bytes (the driver sends everything else through the line passes)
hipError_t launch_fwd_level_i16(Wavelet w, const FwdLevelArgs &a, const SweepTuning &t, hipStream_t s);
hipError_t launch_inv_level_i16(Wavelet w, const InvLevelArgs &a, const SweepTuning &t, hipStream_t s);
// the two sweeps of the float 9/7 on binary16 storage (dwt_sweep2d_h.hip): pitches in 2-byte ELEMENTS, the alignment rule of
// the int16 sweeps
hipError_t launch_fwd_level_h(Wavelet w, const FwdLevelArgs &a, const SweepTuning &t, hipStream_t s);
hipError_t launch_inv_level_h(Wavelet w, const InvLevelArgs &a, const SweepTuning &t, hipStream_t s);
// its line-pass route: a w x h frame of binary16 samples widened into a frame of binary32 ones (exact), or narrowed back
// (round to nearest even); pitches in BYTES
hipError_t launch_half_frame_cvt(bool widen, void *halves, long half_pitch, void *floats, long float_pitch, int w, int h, hipStream_t s);
// true when launch_inv_level has a fused kernel for this wavelet
bool have_fused_inverse(Wavelet w);

// Generic out-of-place 1-D pass over `n_lines` strided lines of length N (exact
// reference semantics for any N; used for sparse frames, single-line directions and
// as the cross-check variant).  Strides in BYTES.  Forward writes L to dst[0..) and
// H to dst[hoff..); inverse reads L from src[0..), H from src[hoff..).
// `lanes_along_lines`: adjacent lanes take adjacent lines (column passes).
hipError_t launch_line_pass(Wavelet w, bool inverse, const void *src, void *dst, long line_stride, long elem_stride,
	int n_lines, int N, int hoff, bool lanes_along_lines, hipStream_t s);

// All levels of a 1-D transform (float 9/7 / 5/3) of `n_lines` lines of N <= N1D_MAX samples in one launch
// (dwt_line1d.hip): line i starts at src + i*line_stride, its elements `elem_stride` bytes apart (a multiple of 4);
// the result (L_J, then the H bands from coarse to fine, Mallat order) goes to the same place in dst, which may be src.
// Forward: `levels` levels from the full line down; inverse: the `levels` coarsest levels back to the full line.
constexpr int N1D_MAX = 8192; // LDS: 56 KiB per line of an inverse at this length -- two workgroups per CU
hipError_t launch_line_levels(Wavelet w, bool inverse, const void *src, void *dst, long line_stride, long elem_stride,
	int n_lines, int N, int levels, hipStream_t s);

// Wavelet packets (dwt_wp1d.hip, dwt_wp2d.hip): every node of a level is split again.  The node tree of
// a line of N samples in natural order: the node [s, s+n) has its L child at [s, s+ceil(n/2)) and its H child behind it;
// index k reads the path from the root, first split in the most significant of its `level` bits (0 = L).
static __host__ __device__ inline void wp_node(int N, int level, int k, int *start, int *len)
{
	int s = 0, n = N;
	for (int b = level - 1; b >= 0; b--) {
		const int nl = (n + 1) >> 1;
		if ((k >> b) & 1) {
			s += nl;
			n -= nl;
		} else
			n = nl;
	}
	*start = s;
	*len = n;
}
// All `levels` packet levels of `n_lines` lines of 2 <= N <= N1D_MAX samples in one launch, 1 <= levels <= floor(log2 N):
// line i at src + i*line_stride, elements `elem_stride` bytes apart (a multiple of 4); the leaves in natural order go to
// the same places in dst, which may be src.  Inverse: the leaves of depth `levels` back to the line.
hipError_t launch_wp_lines(Wavelet w, bool inverse, const void *src, void *dst, long line_stride, long elem_stride, int n_lines,
	int N, int levels, hipStream_t s);
// Pruned packet trees and the best-basis search of lines (dwt_wp_basis.hip).  A tree: WP_TREE_WORDS words,
// bit 2^j + k set = node k of level j is split; only what can be reached from the root through set bits counts.
constexpr int WP_TREE_WORDS = 32, WP_TREE_MAX_LEVELS = 10; // (DWT_HIP_WP_TREE_WORDS, DWT_HIP_WP_TREE_MAX_LEVELS)
enum WpCost { kWpCostShannon = 0, kWpCostLogEnergy = 1, kWpCostLp = 2, kWpCostThreshold = 3 }; // (enum dwt_hip_wp_cost)
// the lines of launch_wp_lines (N <= N1D_MAX, levels <= WP_TREE_MAX_LEVELS) in the tree of each: line i's at tree + i*tree_words
// (tree_words 0: one tree for all), ONE launch
hipError_t launch_wp_tree(Wavelet w, bool inverse, const void *src, void *dst, long line_stride, long elem_stride, int n_lines, int N,
	int levels, const unsigned *tree, long tree_words, hipStream_t s);
struct WpBestArgs {
	const char *src;
	char *dst; // null: costs and tree only
	long line_stride, elem_stride;
	int n_lines, N, levels;
	int tpl, vec; // (set by the launcher)
	int kind;     // WpCost
	float param;
	unsigned *tree;    // null, or line i's at tree + i*tree_words
	long tree_words;
	double *total;     // null, or n_lines doubles
	double *node_cost; // null, or line i's 2^(levels+1) doubles (heap order, [0] = total) at node_cost + i*cost_doubles
	long cost_doubles;
};
// the costs of every node, the best tree and the line in that tree, ONE launch
hipError_t launch_wp_best(Wavelet w, const WpBestArgs &a, hipStream_t s);
// the helpers of the cross-check route: dense frames of n_lines rows `pitch` bytes apart, tables of 2^(levels+1) doubles a line
hipError_t launch_wp_cost_level(const void *frame, long pitch, long n_lines, int N, int j, int kind, float param, double *tab, long tab_doubles,
	hipStream_t s);
hipError_t launch_wp_select(double *tab, long n_lines, int levels, unsigned *tree_ws, unsigned *tree, long tree_words, double *total,
	double *node_cost, long cost_doubles, hipStream_t s);
// mode 0: the samples whose leaf has depth lev; mode 1: depth <= lev
hipError_t launch_wp_leaf_copy(const void *from, void *to, long pitch, long n_lines, int N, int levels, const unsigned *tree, long tree_words,
	int lev, int mode, hipStream_t s);
// One packet level of a batch of dense images, out of place: the 4^level nodes of every W x H image of src are split
// (inverse: rebuilt from their four quarters) into dst.  Strides in BYTES, multiples of 4.
constexpr int WP2D_TILE_W = 128, WP2D_TILE_H = 32; // a workgroup's tile of one node, samples
constexpr int WP2D_MAX_LEVELS = 8;
struct Wp2dLevelArgs {
	const char *src;
	long src_pitch, src_bs;
	char *dst;
	long dst_pitch, dst_bs;
	int W, H, batch, level;
};
bool wp2d_level_fits(const Wp2dLevelArgs &a); // aligned, every node of the level has two samples or more each way, a grid the launch can take
hipError_t launch_wp2d_level(Wavelet w, bool inverse, const Wp2dLevelArgs &a, hipStream_t s);

// Pruned packet QUADTREES and the best-basis search of images (dwt_wp2d.hip, dwt_wp_basis2d.hip).  Node
// (ky, kx) of level j has the index q = (4^j - 1)/3 + ky*2^j + kx; bit q set = the node is split into LL, HL, LH, HH;
// only what can be reached from the root through set bits counts.  A bitmap decides lift-or-copy and never an address.
constexpr int WP_QTREE_WORDS = 16, WP_QTREE_MAX_LEVELS = 5; // (DWT_HIP_WP_QTREE_WORDS, DWT_HIP_WP_QTREE_MAX_LEVELS)
static __host__ __device__ inline int wp_qbase(int j) { return ((1 << (2 * j)) - 1) / 3; } // index of node (0, 0) of level j; nodes of levels 0 .. j-1
// is node (ky, kx) of level j < WP_QTREE_MAX_LEVELS split in the EFFECTIVE tree: its own bit and that of every ancestor
static __host__ __device__ inline bool wp_qtree_split(const unsigned *tree, int j, int ky, int kx)
{
	for (int a = 0; a <= j; a++) {
		const int q = wp_qbase(a) + ((ky >> (j - a)) << a) + (kx >> (j - a));
		if (!((tree[q >> 5] >> (q & 31)) & 1u))
			return false;
	}
	return true;
}
// tiles of `tile` samples along an axis of `size` samples per node of `level`: those of the longest node
static __host__ __device__ inline int wp_tiles(int size, int level, int tile)
{
	const int longest = (size >> level) + ((size & ((1 << level) - 1)) != 0);
	return (longest + tile - 1) / tile;
}
// launch_wp2d_level in trees: image b's at tree + b*tree_words (0: one tree for all).  A workgroup whose node is not split
// in the effective tree copies its tile from src to the same place in dst.  a.level < WP_QTREE_MAX_LEVELS.
struct Wp2dTreeArgs : Wp2dLevelArgs {
	const unsigned *tree;
	long tree_words;
};
hipError_t launch_wp2d_level_tree(Wavelet w, bool inverse, const Wp2dTreeArgs &a, hipStream_t s);
// The cost of every tile of every node of `level` of dense images, the grid of launch_wp2d_level: the tile's terms reduced
// to ONE double in a fixed order, to part[b*part_stride + ((ky*2^level + kx)*nty + ty)*ntx + tx] (ntx, nty: wp_tiles).
struct WpQCostArgs {
	const char *frame;
	long pitch, bs;
	int W, H, batch, level;
	int kind; // WpCost
	float param;
	double *part;
	long part_stride; // doubles between the slots of two images
};
hipError_t launch_wp_qcost_tiles(const WpQCostArgs &a, hipStream_t s);
// the cross-check route's: one thread per (image, node) of `level`, the node's terms in row-major order, to
// tab[b*tab_doubles + q]
hipError_t launch_wp_qcost_level(const void *frame, long pitch, long bs, int W, int H, long batch, int level, int kind, float param, double *tab,
	long tab_doubles, hipStream_t s);
// The selection, all images in one launch.  part not null: tab[b][q] = the node's tile partials of launch_wp_qcost_tiles in
// tile-index order first (the slots of level j of an image begin part_off[j] doubles into its block); null: tab holds the
// costs.  Then bottom-up on a copy; the effective tree to tree_ws (WP_QTREE_WORDS words an image) and, where given, to
// tree; total; node_cost.
struct WpQSelectArgs {
	const double *part;
	long part_stride;
	long part_off[WP_QTREE_MAX_LEVELS + 1];
	double *tab; // batch tables of (4^(levels+1) - 1)/3 doubles, dense
	int W, H, levels, batch;
	unsigned *tree_ws;
	unsigned *tree; // null, or image b's at tree + b*tree_words
	long tree_words;
	double *total;     // null, or batch doubles
	double *node_cost; // null, or image b's table at node_cost + b*cost_doubles
	long cost_doubles;
};
hipError_t launch_wp_qselect(const WpQSelectArgs &a, hipStream_t s);
// one thread per sample of `batch` dense images: copied from `from` to the same place in `to` where the depth d of the
// sample's leaf is lev (mode 0) / at most lev (mode 1)
hipError_t launch_wp_qleaf_copy(const void *from, void *to, long pitch, long bs, int W, int H, long batch, int levels, const unsigned *tree,
	long tree_words, int lev, int mode, hipStream_t s);

// The pixel front end (dwt_pixels.hip): unsigned 8- / 16-bit pixels <-> wavelet planes, one launch per call.
// Channel c of pixel (x, y) of picture b at pix + b*pix_bs + y*pix_pitch + x*pix_stride + c*chan_stride, plane (b, c) at
// planes + (b*channels + c)*plane_stride with rows plane_pitch apart; all in bytes, checked by the driver.
constexpr int PIXELS_PER_LANE = 16;     // consecutive pixels of a row per lane (DWT_HIP_PIXELS_PER_LANE)
constexpr int PIXELS_WG_ROWS = 4;       // rows per workgroup: one per wave
constexpr int PIXELS_GRID_ROWS = 16384; // rows one trip of the kernel's row loop covers (grid.y * PIXELS_WG_ROWS)
constexpr int PIXELS_GRID_BATCH = 4096; // pictures one trip of its batch loop covers (grid.z)
enum PixelPlane { kPlaneI16 = 0, kPlaneI32 = 1, kPlaneH = 2, kPlaneS = 3 }; // (DWT_HIP_PLANE_*)
struct PixelsArgs {
	char *pix;
	long pix_bs, pix_pitch, pix_stride, chan_stride;
	char *planes;
	long plane_stride, plane_pitch;
	int batch, channels, W, H;
	int bgr, colour; // channel 0 of a pixel is B; the component transform of the plane type is applied (RCT / ICT)
	int offset, maxv;
	float scale;
	int layout;   // wide pixel route: 3 / 4 elements per interleaved pixel, 0 one run per channel (planar, grey)
	int wide_pix, wide_planes; // that side moves by 16-byte accesses (pixels_route)
	int pix_al2;  // element route: 16-bit pixels lie on even addresses
	int nt_out;   // the wide stores are non-temporal
};
hipError_t launch_pixels(int pix_bytes, int plane, bool inverse, const PixelsArgs &a, hipStream_t s);

// Edge-avoiding 5/3 and 9/7 (dwt_eaw.hip).  One exact pass over n_lines lines (line l at src + l*ls, elements es bytes
// apart, a multiple of 4) into the dense scratch tmp (n_lines x N floats, sample order); weights w[l*N + i] written
// (forward) or read (inverse).  hoff: where the line's H half starts (Mallat), or -1 (interleaved: sample i at i).  The
// inverse reads its input at those places; launch_eaw_place then moves tmp to its places in the lines (forward: Mallat /
// interleaved places, inverse: hoff = -1).
enum EawWavelet { kEaw53, kEaw97 };
hipError_t launch_eaw_line(EawWavelet wv, bool inverse, const void *src, long ls, long es, int n_lines, int N, int hoff, float *tmp,
	float *w, bool lanes_along_lines, float alpha, hipStream_t s);
hipError_t launch_eaw_place(void *dst, long ls, long es, int n_lines, int N, int hoff, const float *tmp, bool lanes_along_lines, hipStream_t s);
// One fused level of a dense Mallat frame (W, H >= 2), `batch` images bi_* floats apart; pitches in floats.
// Forward: in -> LL to ll_out, the detail subbands to det_out at their Mallat places, weights to wH_out (H x W) /
// wV_out (W x H, column-major).  Inverse: LL from ll, details from det, weights from wH / wV -> out.
struct EawLevelArgs {
	const float *in = nullptr;
	float *ll_out = nullptr, *det_out = nullptr, *wH_out = nullptr, *wV_out = nullptr;
	const float *ll = nullptr, *det = nullptr, *wH = nullptr, *wV = nullptr;
	float *out = nullptr;
	long pin = 0, pll = 0, pd = 0, pout = 0;
	long bi_in = 0, bi_ll = 0, bi_det = 0, bi_w = 0, bi_out = 0;
	int W = 0, H = 0, batch = 1;
};
hipError_t launch_eaw_level(EawWavelet wv, bool inverse, const EawLevelArgs &a, float alpha, hipStream_t s);

// z-pass knobs of the 3-D path (measured defaults; options vol_cpt / vol_tile_pairs / vol_nt)
struct VolTuning {
	int cpt = 8;        // columns per lane: 4 or 8 (two groups of 4, 256 columns apart; +4 % at 1024^3)
	int tile_pairs = 0; // slice pairs per wave; 0 = choose from the volume depth
	int nt = -1;        // bit 0 non-temporal stores, bit 1 non-temporal loads; -1 = measured default
	                    // (z pass: 0, fused level: stores non-temporal, +9 %)
	int inplace_fused = 1; // in-place calls: 1 = one fused pass per level in place over a snapshot of the tile halos (forward and inverse),
	                       // 0 = two passes per level (the cross-check)
	int whole = 1;      // whole-tile variant of the fused kernel where the volume allows (0: the general one)
	int direct = 2;     // fused levels >= 1 write into their lattice of the destination: 2 = level 1 merged with level 0's withheld rows where the sizes allow, 1 = strided stores, 0 = dense volume + scatter pass
	int fused = 1;      // out-of-place forward levels: 1 = one fused pass where it pays, 2 = wherever it can run, 0 = two passes
	int swizzle = 1;    // fused level: hand contiguous runs of tiles to one XCD
	int rows = 8;       // fused level: output rows per wave, 8 (measured best) or 6 (two workgroups per CU)
	int ip_waves = 0;   // k_vol_level_ip: waves per workgroup, 4 (tiles of 32 rows, two workgroups per CU) or 8 (64 rows, one); 0 = 8 where the volume has more than 32 rows
};

// z pass of the 3-D path: CDF 9/7 float along the slice axis of an interleaved volume,
// out of place (in != out), x dense; strides in ELEMENTS.  Forward only: when `lll` is set the
// even-x/even-y/even-z samples (the next level's input) are also written densely there.
hipError_t launch_vol_z(bool inverse, const float *in, long in_sy, long in_sz, float *out, long out_sy, long out_sz,
	int nx, int ny, int nz, const VolTuning &vt, hipStream_t s, float *lll = nullptr, long lll_sy = 0, long lll_sz = 0);

// One forward 3-D level in ONE pass, out of place (in != out): x, y and z lifting fused.  A
// workgroup owns 256 x 32 voxel columns and marches along z; see k_vol_fwd_fused.  Applies
// to volumes at least 128 samples wide with about one workgroup per CU (vol_fused_applies);
// overhanging or unaligned tiles are staged column by column.
struct VolFusedArgs {
	const float *in;
	long in_sy, in_sz;
	float *out;
	long out_sy, out_sz;
	float *lll; // optional dense copy of the even-even-even samples (next level's input)
	long lll_sy, lll_sz;
	int nx, ny, nz;
	// multi-level store variants (see k_vol_fwd_fused): 1 = level j >= 1 into its lattice of the
	// destination (out_sx = 2^j, out_sy / out_sz the destination's strides times 2^j); 2 = level 0
	// withholding its even-y even-z rows (odd-x samples to `side`, laid out like `lll`); 3 = level 1
	// writing those rows whole (out_sy / out_sz the destination's strides times 2; `side` read)
	int mode = 0;
	long out_sx = 1;
	int temporal_shared = 0; // mode 3: the rows the next level's merge pass reads again are stored temporal
	float *side = nullptr;
	long side_sy = 0, side_sz = 0;
};
bool vol_fused_applies(const VolFusedArgs &a);
hipError_t launch_vol_fwd_fused(const VolFusedArgs &a, const VolTuning &vt, hipStream_t s);

// One 3-D level in ONE pass and IN PLACE (in == out, same strides), forward or inverse
// (dwt_vol3d_ip.hip): a snapshot of the SHELL -- the rows, columns and slices a tile of the fused
// kernel reads but does not own, about a quarter of the volume -- is taken into `scratch`
// (vol_level_ip_scratch bytes), then the fused kernel reads tile interiors from the volume and halos
// from the shell.  mode 0 (dense rows) or, forward only, 2 (see VolFusedArgs); `lll` as above.
struct VolShell {
	float *rs; // rows: [nz][7 (tile rows - 1)][nx]
	long rs_sy, rs_sz;
	float *cs; // columns: [nz][ny][8 (tile columns - 1)]
	long cs_sy, cs_sz;
	float *zs; // slices: [9 (marches - 1) + 5][ny][nx]
	long zs_sy, zs_sz;
	int tile_pairs_z, nzt; // slice pairs per march, marches along z
};
bool vol_level_ip_can(const VolFusedArgs &a);     // the kernel can run (any size from 2 x 2 x 8)
bool vol_level_ip_applies(const VolFusedArgs &a); // ... and pays
size_t vol_level_ip_scratch(const VolFusedArgs &a, const VolTuning &vt);
hipError_t launch_vol_level_ip(bool inverse, const VolFusedArgs &a, float *scratch, const VolTuning &vt, hipStream_t s);
// the same kernel OUT OF PLACE (in != out, dense source, no shell).  Forward: mode 0 / 2 and `lll` as for
// launch_vol_fwd_fused (tiles of 64 rows where the volume has them).  Inverse: mode 0 dense result, mode 1
// result into the stride-out_sx lattice of `out` (a level >= 1 of a multi-level inverse).
hipError_t launch_vol_level_op(bool inverse, const VolFusedArgs &a, const VolTuning &vt, hipStream_t s);

// Strided 3-D copy (lattice pack/unpack for the levels >= 1 of the 3-D path);
// strides in ELEMENTS, including the x strides.
hipError_t launch_lattice_copy(const float *src, long s_sx, long s_sy, long s_sz, float *dst, long d_sx, long d_sy, long d_sz,
	int nx, int ny, int nz, hipStream_t s);
// the same for a dense source and a destination whose rows hold dst_nx samples: strides 2 and 4 as
// a read-modify-write of whole 16-byte pieces where they fit the rows
hipError_t launch_lattice_scatter(const float *src, long s_sy, long s_sz, float *dst, long d_sx, long d_sy, long d_sz,
	int nx, int ny, int nz, int dst_nx, hipStream_t s);

// One PHASE of the reference's phase-ordered in-place lifting (src/dwt-simple.c:2266-2350,
// src/libdwt.c:17517-17594): lifting step s updates the coefficients lo[s]..hi[s] of its
// parity only, the scaling touches sc_lo..sc_hi only; everything else is copied.  Out of
// place, one thread per coefficient pair, interleaved layout on both sides.
struct IlPhase {
	int lo[4], hi[4];
	int sc_lo, sc_hi;
};
// k_lo / k_hi: only the coefficient pairs k_lo .. k_hi-1 of every line are computed and written
// (k_hi < 0: to the end of the line) -- the exact border strips of the fused interleaved path.
hipError_t launch_il_phase(Wavelet w, bool inverse, const void *src, void *dst, long line_stride, long elem_stride,
	int n_lines, int N, bool lanes_along_lines, const IlPhase &ph, hipStream_t s, int k_lo = 0, int k_hi = -1);

// The two exact border strips of a fused interleaved level (k_il_strip, one launch): the level's input (odd rows at
// `in`, even rows there too or packed at `in_even`), the sweep's output `out` it corrects, the
// optional dense low-pass copy `ll`; pitches in ELEMENTS; rph / cph: the prolog, core and epilog
// ranges of the row (N = lx) and column (N = ly) transforms.
struct IlStripArgs {
	const float *in;
	long in_pitch;
	int in_step;         // elements between neighbouring samples of an input row (a level on its lattice in a larger image)
	const float *ll_in;  // or null: dense low-pass band that replaces the input samples at (even row, even column)
	long ll_in_pitch;
	const float *top_in;   // or null (in-place level): rows 0 .. 13 of the input, IlShell::top
	long top_in_pitch;
	const float *right_in; // or null (in-place level): columns right_x0 .. of every input row, IlShell::right
	long right_in_pitch;
	int right_x0;
	float *out;
	long out_pitch;
	int out_step; // elements between neighbouring samples of an output row
	float *ll;
	long ll_pitch;
	int lx, ly;
	IlPhase rph[3], cph[3];
};


// Up to three device-to-device rectangle copies in one launch; widths in BYTES (multiples of 4).
struct CopyRects {
	const char *src[3];
	char *dst[3];
	long spitch[3], dpitch[3];
	int wbytes[3], h[3];
	int first_block[4];
	int n;
	int policy = 3; // 3: non-temporal loads and stores (data moved once); 0: temporal both ways (the copy is read again at once)
	int block0 = 0; // a launch's workgroup b copies block block0 + b
};
hipError_t launch_copy_rects(CopyRects r, hipStream_t s);
// the same copy cut into blocks of 8 rows x 4 KiB: fills first_block / n, returns the number of blocks (< 0: bad
// arguments); launch_copy_rects_range runs blocks [lo, hi) as a launch of their own
int copy_rects_plan(CopyRects *r);
hipError_t launch_copy_rects_range(CopyRects r, int lo, int hi, hipStream_t s);

// Per-subband feature statistics (dwt_features.hip).  Every kernel leaves RAW results per (image, band)
// record in planes of 8 bytes (plane f of record r at rec[f * nrec + r]): sums as doubles, accumulated in a fixed order
// that depends on the band geometry alone, never on the launch geometry; the host finishes them in float.
enum FeatPlane { kFeatS1, kFeatS2, kFeatSp, kFeatM2, kFeatM3, kFeatM4, kFeatKey /* max |x| bits << 32 | ~first index */, kFeatMed /* float bits */, kFeatPlanes };
enum FeatWork { kFeatPass2 = 1, kFeatSelect = 2 };
// how the kernels form the term of plane kFeatSp: nothing, |x|, or (float)pow((double)|x|, (double)p)
enum FeatPmode { kFeatPNone, kFeatPAbs, kFeatPPow };
// one band of an image, cut into slabs of <= cw columns x rh rows (column chunk fastest); slab0: its first slab within the image
struct FeatBand {
	int x0, y0, w, h;
	int cw, rh, ncc, nslab, slab0;
};
constexpr int FEAT_MAX_BANDS = 96;
constexpr int FEAT_SLAB = 16384, FEAT_SLAB_COLS = 4096; // elements per slab, widest slab
struct FeatLineArgs {
	const char *src;
	long line_stride; // bytes
	int n_lines, N, nb;
	int off[32], len[32]; // band k of a line: samples off[k] .. off[k] + len[k]
	unsigned long long *rec;
	long nrec;
	int work, pmode;
	float p;
};
// dense lines of N <= N1D_MAX floats, one workgroup per line, every band and every statistic in ONE launch
hipError_t launch_feat_lines(const FeatLineArgs &a, hipStream_t s);
struct FeatImgArgs {
	const char *img;
	long pitch, bstride; // bytes
	int batch, nb, slabs; // bands and slabs of ONE image
	const FeatBand *bands; // device table
	unsigned long long *part; // 4 planes of batch * slabs partials
	unsigned long long *rec;
	long nrec;
	unsigned *hist; // 4 passes x nrec x 256 bins, zeroed by the caller
	unsigned *sel;  // nrec x {prefix, rank}
	int pmode;
	float p;
	int use_c, mn; // pass 2 about c instead of the band's mean; mn outside 2..4: plane kFeatM2 takes (float)pow(x - c, mn)
	float c;
	int groups; // workgroups of the slab passes
	int abs_key; // the select orders |x| instead of x (the key ignores the sign bit): the median magnitude, the band untouched
};
hipError_t launch_feat_pass1(const FeatImgArgs &a, hipStream_t s); // -> part planes 0..3
hipError_t launch_feat_pass2(const FeatImgArgs &a, hipStream_t s); // -> part planes 0..2
hipError_t launch_feat_fold(const FeatImgArgs &a, int second, hipStream_t s); // part -> rec (first: S1 S2 Sp Key; second: M2 M3 M4)
hipError_t launch_feat_hist(const FeatImgArgs &a, int pass, hipStream_t s);
hipError_t launch_feat_pick(const FeatImgArgs &a, int pass, hipStream_t s);
// |x| in place over w x h floats, element (y, x) at y*sx + x*sy bytes
hipError_t launch_feat_abs(void *p, long sx, long sy, int w, int h, hipStream_t s);

// Per-band coefficient operators (dwt_bandops.hip): one operator and one parameter per slot of a Mallat
// frame -- slot 3(j-1) + {0, 1, 2} is HL, LH, HH of level j, the last slot LL of the deepest level -- applied in place to
// every image of a batch in ONE launch.  The ops are those of enum dwt_hip_band_op, then the two pointwise maps.
enum BandOp { kBandKeep = 0, kBandZero, kBandScale, kBandHard, kBandSoft, kBandCompress, kBandOps, kMapLog = kBandOps, kMapExp, kBandOpsAll };
constexpr int BAND_MAX_SLOTS = 94; // 3 * 31 + 1
constexpr int BAND_CHUNK = 16384, BAND_CHUNK_COLS = 4096; // elements per workgroup chunk, widest chunk
// a band of w x h elements is cut into chunks of band_chunk_cols(w) columns x band_chunk_rows(w) rows, column chunk fastest
static __host__ __device__ inline int band_chunk_cols(int w) { return w < BAND_CHUNK_COLS ? w : BAND_CHUNK_COLS; }
static __host__ __device__ inline int band_chunk_rows(int w) { return w < 1 ? 1 : BAND_CHUNK / band_chunk_cols(w); }
struct BandOpsArgs {
	char *img;           // dense images of 4-byte elements
	long pitch, bstride; // bytes
	int batch, nslots;
	int x0[BAND_MAX_SLOTS], y0[BAND_MAX_SLOTS], w[BAND_MAX_SLOTS], h[BAND_MAX_SLOTS];
	int first[BAND_MAX_SLOTS + 1]; // prefix of the slots' chunk counts within one image (a slot no image touches: none)
	unsigned char op[BAND_MAX_SLOTS + 2];
	float param[BAND_MAX_SLOTS];
	// per-image tables (device memory; null: the one table above): image b reads entry b * tstride + slot
	const int *dev_op;
	const float *dev_param;
	long tstride;
};
hipError_t launch_band_ops(const BandOpsArgs &a, hipStream_t s);

// Deadzone quantization of coefficient planes (dwt_quant.hip): float coefficients <-> sign-magnitude
// indices, one step per slot of a dense Mallat frame, one launch per call.  Sample (x, y) of frame b at
// coef + b*coef_bs + y*coef_pitch + x*(coef element) and index + b*index_bs + y*index_pitch + x*(index element), bytes.
constexpr int QUANT_WG_ROWS = 4;       // rows per workgroup: one per wave
constexpr int QUANT_GRID_ROWS = 16384; // rows one trip of the kernel's row loop covers (grid.y * QUANT_WG_ROWS)
constexpr int QUANT_GRID_BATCH = 4096; // frames one trip of its batch loop covers (grid.z)
constexpr int QUANT_MAX_LEVELS = 31;
constexpr int QUANT_STAT_WORDS = 3;    // per slot: nonzero indices, largest magnitude, clipped samples
enum QuantCoef { kCoefS = 0, kCoefH = 1 };      // (DWT_HIP_COEF_*)
enum QuantIndex { kIndexI16 = 0, kIndexI32 = 1 }; // (DWT_HIP_INDEX_*)
constexpr int quant_coef_es(int t) { return t == kCoefH ? 2 : 4; }
constexpr int quant_index_es(int t) { return t == kIndexI16 ? 2 : 4; }
// samples of a lane's run: the narrower side is one 16-byte access
constexpr int quant_run(int coef, int index) { return 16 / (quant_coef_es(coef) < quant_index_es(index) ? quant_coef_es(coef) : quant_index_es(index)); }
struct QuantArgs {
	char *coef;
	long coef_pitch, coef_bs;
	char *index;
	long index_pitch, index_bs;
	int batch, W, H, J;
	// xb[j], yb[j]: the first column / row of the H half of level j = 1 .. J (the band table's x of HL(j), y of LH(j));
	// a position's column level is the smallest j with x >= xb[j], J + 1 (L) where there is none; rows alike
	int xb[QUANT_MAX_LEVELS + 1], yb[QUANT_MAX_LEVELS + 1];
	const float *tab; // device: frame b reads tab[b*tstride + slot] -- 1 / step (quantize), step (dequantize)
	long tstride;
	float r;          // dequantize: the reconstruction offset
	// quantize: null, or QUANT_STAT_WORDS counters per slot per frame per copy, cleared before the launch; workgroups
	// spread over stat_copies (a power of two) copies, which the driver folds
	unsigned long long *stats;
	int stat_copies;
	int wide_coef, wide_index; // that side moves by 16-byte accesses (quant_route)
	int nt_out;                // the wide stores are non-temporal
};
hipError_t launch_quant(int coef, int index, bool inverse, const QuantArgs &a, hipStream_t s);
// The magnitude bit-planes of every code-block: a band of slot k is cut into blocks of (1 << cbx) x (1 << cby) samples from
// its first sample on; planes[b*planes_bs + first[k] + by*blocks_x[k] + bx] = bit length of the block's largest |q|.
constexpr int CODEBLOCK_WG_BLOCKS = 4;      // code-blocks per workgroup: one per wave
constexpr int CODEBLOCK_GRID = 16384;       // workgroups of one trip of the kernel's loop
struct CodeblockArgs {
	const char *index;
	long index_pitch, index_bs;
	int batch, nslots, cbx, cby;
	int wide; // base, row pitch and batch stride are multiples of 16 bytes: rows are read by 16-byte chunks
	int x0[BAND_MAX_SLOTS], y0[BAND_MAX_SLOTS], w[BAND_MAX_SLOTS], h[BAND_MAX_SLOTS];
	int first[BAND_MAX_SLOTS + 1]; // prefix of the slots' block counts
	int blocks_x[BAND_MAX_SLOTS];
	unsigned char *planes;
	long planes_bs;
};
hipError_t launch_codeblock_bitplanes(int index, const CodeblockArgs &a, hipStream_t s);

// Sparse coefficient streams (dwt_sparse.hip): the kept elements of dense Mallat frames as (position,
// value) entries in stream order, and back.  Element (x, y) of frame b at planes + b*bs + y*pitch + x*es bytes.  A frame is
// cut into tiles of SPARSE_TILE_SAMPLES consecutive samples of one band's raster order, enumerated in stream order
// (dwt_sparse_geom.c); the band table rides in the kernel arguments.
constexpr int SPARSE_TILE_SAMPLES = 2048;
constexpr int SPARSE_GRID_TILES = 4096; // tiles one trip of the tile loop covers (grid.x); the scatter's workgroups alike
constexpr int SPARSE_GRID_BATCH = 4096; // frames one trip of the batch loop covers (grid.y)
struct SparseArgs {
	const char *planes;
	long pitch, bs;
	int batch, W, H;
	int bands, tiles;   // 3J + 1 bands in stream order; tiles of one frame
	unsigned keep_mask; // an element is kept when (bits & keep_mask) != 0: everything but a float's sign bit
	int wide;           // base, pitch and batch stride are multiples of 16 bytes
	int x0[BAND_MAX_SLOTS], y0[BAND_MAX_SLOTS], w[BAND_MAX_SLOTS], h[BAND_MAX_SLOTS];
	int first[BAND_MAX_SLOTS + 1]; // prefix of the bands' tile counts
	unsigned *tile;               // [batch][tiles]: launch 1 the tiles' counts, launch 2 the tiles' first entries
	unsigned *pos;                 // frame b's entries from b * stream_stride on
	char *val;
	unsigned long long stream_stride;
	unsigned *offsets; // [batch][bands + 1]
};
hipError_t launch_sparse_tiles(int es, bool pack, const SparseArgs &a, hipStream_t s); // launch 1 / launch 3
hipError_t launch_sparse_scan(const SparseArgs &a, hipStream_t s);                     // launch 2
struct SparseUnpackArgs {
	char *planes;
	long pitch, bs;
	int batch, W, H;
	int wide, nt; // 16-byte stores; non-temporal ones
	const unsigned *pos;
	const char *val;
	unsigned long long stream_stride;
	const unsigned *counts;
	long counts_stride; // in words
};
hipError_t launch_sparse_zero(int es, const SparseUnpackArgs &a, hipStream_t s);
hipError_t launch_sparse_scatter(int es, const SparseUnpackArgs &a, hipStream_t s);

// Embedded bit-plane streams of code-blocks (dwt_bitplane.hip): every code-block of an index frame as a
// sign plane and its magnitude planes, most significant first, in 64-bit words of 64 samples.  Sample (x, y) of frame b at
// index + b*bs + y*pitch + x*es bytes.  The bands ride in the kernel arguments in STREAM order (dwt_bitplane_geom.c), with
// the prefix of their block counts.
constexpr int BITPLANE_WG_BLOCKS = 4;      // launch 1: code-blocks per workgroup, one per wave
constexpr int BITPLANE_GRID_BLOCKS = 16384; // blocks one trip of the pack / unpack kernels' loops covers (one per workgroup); launch 1: workgroups
constexpr int BITPLANE_GRID_BATCH = 4096;  // frames one trip of the scan's loop covers
constexpr int BITPLANE_MAX_WORDS = 33 * 64; // of one block: 33 planes of 4096 samples
enum BitplaneMode { kBitplaneKeep = 0, kBitplaneShift = 1 }; // (DWT_HIP_BITPLANE_*)
struct BitplaneArgs {
	char *index;
	long pitch, bs;
	int batch, bands, blocks; // 3J + 1 bands in stream order; blocks of one frame
	int cbx, cby;
	int wide; // launch 1, unpack: base, pitch and batch stride are multiples of 16 bytes (16-byte reads of launch 1, 16-byte stores of unpack)
	int x0[BAND_MAX_SLOTS], y0[BAND_MAX_SLOTS], w[BAND_MAX_SLOTS], h[BAND_MAX_SLOTS];
	int first[BAND_MAX_SLOTS + 1]; // prefix of the bands' block counts
	int blocks_x[BAND_MAX_SLOTS];
	unsigned *sizes;   // [batch][blocks]: the blocks' sizes in words (launch 1 -> launch 2)
	unsigned *offsets; // [batch][blocks + 1]
	unsigned long long *words; // frame b's from b * stream_stride on
	unsigned long long stream_stride;
	int drop, mode, nt; // unpack: planes left out, KEEP / SHIFT, non-temporal stores
};
hipError_t launch_bitplane_sizes(int index, const BitplaneArgs &a, hipStream_t s);             // launch 1
hipError_t launch_bitplane_scan(const BitplaneArgs &a, hipStream_t s);                         // launch 2
hipError_t launch_bitplane_pack(int index, bool wave, const BitplaneArgs &a, hipStream_t s);   // launch 3
hipError_t launch_bitplane_unpack(int index, bool wave, const BitplaneArgs &a, hipStream_t s);

// User-defined lifting wavelets (dwt_lifting.hip): the caller's scheme as the kernels take it, by value in
// the kernel arguments (wave-uniform).  Samples are 4-byte words (binary32 or int32); pitches and batch strides below are
// in ELEMENTS.
constexpr int LIFT_MAX_STEPS = 8, LIFT_MAX_TERMS = 4;
constexpr int LIFT_TILE = 64;       // side of a workgroup's tile of the level
constexpr int LIFT_FUSED_REACH = 8; // the largest halo the tile kernels stage
struct LiftStep {
	int parity, n_terms, reach; // reach: the largest |offset| of the step
	int sign, add, shift;       // int schemes
	int off_a[LIFT_MAX_TERMS], off_b[LIFT_MAX_TERMS];
	float coef[LIFT_MAX_TERMS];
	int num[LIFT_MAX_TERMS];
};
struct LiftTable {
	int is_int, n_steps, inv_cols_first, reach;
	float fwd_scale[2], inv_scale[2];
	LiftStep steps[LIFT_MAX_STEPS];
};
// One fused level on the W x H rectangle.  Forward: `in` -> LL to `out`, HL / LH / HH to `det` at their Mallat offsets of
// the rectangle.  Inverse: LL from `in`, HL / LH / HH from `det` -> the W x H result to `out`.  No tile reads what another
// writes: `in` and `det` (inverse) share no element with `out` and `det` (forward).
struct LiftLevelArgs {
	int W, H, batch;
	const void *in;
	long pin, bi_in;
	void *det;
	long pd, bi_det;
	void *out;
	long pout, bi_out;
};
hipError_t launch_lift_tile(bool inverse, const LiftTable &tb, const LiftLevelArgs &a, hipStream_t s);
// the step-by-step route on a dense scratch x[batch][H][W]
hipError_t launch_lift_copy(const void *src, long ps, long bs, void *dst, long pd, long bd, int W, int H, int batch, hipStream_t s);
hipError_t launch_lift_step(bool is_int, bool inverse, void *x, int W, int H, int batch, const LiftStep &st, bool rows, hipStream_t s);
hipError_t launch_lift_scale(void *x, int W, int H, int batch, bool along_x, float f0, float f1, hipStream_t s);
// x -> the four subbands at their Mallat places of dst's W x H rectangle, scaled by the parity of y (scale: float schemes)
hipError_t launch_lift_place(const void *x, void *dst, long pd, long bd, int W, int H, int batch, bool scale, float f0, float f1, hipStream_t s);
// LL (from ll) and HL / LH / HH (from det) of the W x H rectangle -> x in sample order, scaled by the parity along x or y
hipError_t launch_lift_gather(const void *ll, long pll, long bll, const void *det, long pd, long bd, void *x, int W, int H, int batch,
	bool scale, bool along_x, float f0, float f1, hipStream_t s);
// Every level of `n_lines` lines of N <= N1D_MAX samples in ONE launch (k_lift_lines), any reach: line i at
// src + i*line_stride, elements `elem_stride` bytes apart (multiples of 4); the result in the 1-D Mallat order of
// launch_line_levels goes to the same places in dst, which may be src.  Forward: `levels` levels from the full line down;
// inverse: the `levels` coarsest levels back to the full line.  Lines of up to LIFT_LINE_WAVE samples get a wave each,
// up to LIFT_LINE_HALF half a workgroup, longer ones the whole of it.
constexpr int LIFT_LINE_WAVE = 512, LIFT_LINE_HALF = 2048;
hipError_t launch_lift_lines(bool inverse, const LiftTable &tb, const void *src, void *dst, long line_stride, long elem_stride, int n_lines,
	int N, int levels, hipStream_t s);
// the step-by-step route of lines: W words of H lines, element i of line y at y*ls + i*es WORDS (source: sls, ses; dst:
// dls, des).  mode 0: a copy (ll).  mode 1: Mallat order (L from ll, H from det, both by the source's strides) -> sample
// order; mode 2: sample order (ll) -> Mallat order; scale: times f0 / f1 by the parity of the sample (float schemes)
hipError_t launch_lift_line_move(int mode, const void *ll, const void *det, long sls, long ses, void *dst, long dls, long des, int W, int H,
	bool scale, float f0, float f1, hipStream_t s);

// N-term approximation (dwt_nterm.hip): keep the coefficients of the n largest magnitudes of every group
// of 1 .. 4 dense frames, zero the rest.  The key of a position is the uint32 image of its float magnitude (sign bit 0:
// unsigned order is float order); a radix select over 11 + 10 + 10 bits finds the key of descending rank n, one
// histogram launch per digit, and the apply launch zeroes what lies below it.  Per group the workspace holds
// NTERM_HIST counters (the three digits' histograms one after the other, cleared before the call) and NTERM_REC words:
// digit and remaining rank after the first and after the second narrowing, then the threshold's bits and the kept count.
constexpr int NTERM_MAX_CH = 4;
constexpr int NTERM_BINS0 = 2048, NTERM_BINS1 = 1024, NTERM_BINS2 = 1024, NTERM_HIST = NTERM_BINS0 + NTERM_BINS1 + NTERM_BINS2;
constexpr int NTERM_REC = 8;
constexpr int NTERM_SLAB = 16384; // elements of one channel per slab of rows, about
struct NtermArgs {
	char *img;                    // channel c of group g at img + g*bstride + c*cstride, rows `pitch` bytes apart
	long pitch, bstride, cstride; // bytes
	int batch, channels, w, h;
	int lx, ly;           // positions x < lx && y < ly are outside the scope (0, 0: the whole frame is inside)
	int slab_rows, slabs; // rows per slab, slabs per group
	int bpg;              // workgroups per group: workgroup i walks slabs i % bpg, i % bpg + bpg, .. of group i / bpg
	int vec;              // every base, pitch and stride is a multiple of 16 bytes: whole quads as 16-byte accesses
	const unsigned *rank; // per group: the descending rank asked for, 1 .. positions in scope
	unsigned *hist;       // batch * NTERM_HIST
	unsigned *rec;        // batch * NTERM_REC
	char *map;            // magnitude launch only: the map of group g at map + g*map_bstride
	long map_pitch, map_bstride;
};
hipError_t launch_nterm_hist(const NtermArgs &a, int pass, hipStream_t s); // pass 0, 1, 2
hipError_t launch_nterm_apply(const NtermArgs &a, hipStream_t s);
hipError_t launch_nterm_magnitude(const NtermArgs &a, hipStream_t s);

// Conditioning of rows (dwt_condition.hip): median shift, centring, range scaling.  The bits are those of
// enum dwt_hip_rows_op; a row's record is 4 ints: net offset, moves made, last centre found (-1: none), SCALE skipped it.
enum CondOp { kCondMedShift = 1, kCondCenter = 2, kCondScale = 4 };
struct CondLineArgs {
	char *ptr;        // dense rows of N <= N1D_MAX floats, conditioned in place
	long line_stride; // bytes
	int n_lines, N;
	unsigned ops;
	int max_iters;
	float lo, hi;
	int *info; // device memory, 4 ints per row, or null
	int *warn; // device memory, two counters the centre evaluations add to: zero norm, crossing not found
	int vec;   // 16-byte accesses of the rows are aligned
	int rows;  // rows per workgroup (set by the launcher: cond_rows_per_group, at most n_lines)
};
int cond_rows_per_group(int N);
// all the operations of `ops`, in the order of their bits, in ONE launch
hipError_t launch_cond_lines(CondLineArgs a, hipStream_t s);
// the per-operation kernels: sample i of row y at p + y*ls + 4*i, any N >= 1; per-row results in device memory
hipError_t launch_rows_median(const char *p, long ls, int n_lines, int N, float *med, hipStream_t s);
hipError_t launch_rows_minmax(const char *p, long ls, int n_lines, int N, float *mn, float *mx, hipStream_t s);
// center[y]; displ[y] = center - N/2, info updated as by one iteration of center1, *moved set if any row moves (each optional);
// warn: two counters added to (zero norm, crossing not found); skip_done: rows whose displ is 0 are not looked at again
hipError_t launch_rows_center(const char *p, long ls, int n_lines, int N, int *center, int *displ, int *info, int *moved, int *warn,
	int skip_done, hipStream_t s);
// dst[x] = src[x + d] (d = displ[y], or displ_all), outside the row zero (zero_fill) or the nearest sample; src != dst
hipError_t launch_rows_displace(const char *src, long sls, char *dst, long dls, int n_lines, int N, const int *displ, int displ_all,
	int zero_fill, hipStream_t s);
// element (y, x) at p + y*sx + x*sy.  op 0: += a; 1: *= a; 2: += -v[y]; 3: scale21 to [a, b] from min v[y] and max v2[y],
// the skip flag into info[4*y + 3] (info optional)
hipError_t launch_elem_op(char *p, long sx, long sy, int w, int h, int op, float a, float b, const float *v, const float *v2, int *info,
	hipStream_t s);
hipError_t launch_info_init(int *info, int n_lines, hipStream_t s);

// The stationary (undecimated) wavelet transform of rows (dwt_swt1d.hip): level l filters the previous
// level's low-pass plane with both filters dilated by 1 << (level0 + l), borders replicated; every plane has N samples.
constexpr int SWT_MAX_LEVELS = 24; // level0 + levels <= 24: (half a filter) << level stays far inside int
enum SwtBorder { kSwtReplicate = 0, kSwtSymmetric = 1 }; // DWT_HIP_SWT_BORDER_*: clamp (the reference's), whole-sample reflection (invertible)
struct SwtLineArgs {
	const char *src;  // dense lines of N <= N1D_MAX floats
	long line_stride; // bytes
	int n_lines, N, level0, levels, vec; // vec: 16-byte loads of the line are aligned
	// coefficient mode: H of level l of line y at dst_h + l*plane_stride + y*dst_line_stride, dense; L by l_mode (0: none,
	// 1: the last level's at plane 0, 2: every level's like H)
	char *dst_h, *dst_l;
	long plane_stride, dst_line_stride;
	int l_mode;
	// feature mode: nothing but the records of (line, level), r = line * levels + l, planes as FeatPlane
	unsigned long long *rec;
	long nrec;
	int band; // 0: the H planes, 1: the L planes
	int work, pmode;
	float p;
	int border; // SwtBorder (coefficient mode; feature mode is replicate only)
};
// every level of every line in ONE launch, the L chain in LDS
hipError_t launch_swt_lines(Wavelet w, bool features, const SwtLineArgs &a, hipStream_t s);
// one level through global memory, one thread per output sample: element i of line y at base + y*ls + i*es (bytes) on
// every side; out_l, out_l2 and out_h may each be null
struct SwtLevelArgs {
	const char *src;
	long src_ls, src_es;
	int n_lines, N, level;
	char *out_l, *out_l2, *out_h;
	long l_ls, l_es, l2_ls, l2_es, h_ls, h_es;
	int border; // SwtBorder
};
hipError_t launch_swt_level(Wavelet w, const SwtLevelArgs &a, hipStream_t s);

// The stationary wavelet transform of image batches (dwt_swt2d.hip): one level at dilation 1 << level,
// the row pass (Lr, Hr along x) and then the column pass (LL, LH from Lr; HL, HH from Hr along y).  Every plane is W x H.
constexpr int SWT2D_TILE_W = 256, SWT2D_TILE_H = 32; // the fused kernel's tile: columns, rows of the level's row lattice
constexpr int SWT2D_FUSED_LEVELS = 5;                // ... which runs levels 0 .. 4 (dilations 1 .. 16)
struct Swt2dLevelArgs {
	const char *src; // element (x, y) of image b at src + b*src_bs + y*src_sx + x*src_sy (bytes)
	long src_bs, src_sx, src_sy;
	int W, H, batch, level;
	char *ll, *hl, *lh, *hh; // ll may be null (no LL stored)
	long ll_bs, ll_sx;       // LL has its own batch stride and pitch (the chain's scratch image, or the caller's plane)
	long d_bs, d_sx;         // HL, LH, HH
	long d_sy;               // the element stride of all four outputs
	char *lr, *hr;           // the two passes: dense scratch planes, pitch 4*W, image b at + b*H*4*W
	int border;              // SwtBorder
};
bool swt2d_fused_fits(const Swt2dLevelArgs &a); // dense elements, level below SWT2D_FUSED_LEVELS, a grid the launch can take
hipError_t launch_swt2d_fused(Wavelet w, const Swt2dLevelArgs &a, hipStream_t s); // one launch: src read once, four planes written once
hipError_t launch_swt2d_rows(Wavelet w, const Swt2dLevelArgs &a, hipStream_t s);  // src -> lr, hr; one thread per sample, any strides
hipError_t launch_swt2d_cols(Wavelet w, const Swt2dLevelArgs &a, hipStream_t s);  // lr, hr -> ll, hl, lh, hh

// The inverse stationary transforms under the symmetric border (dwt_iswt1d.hip, dwt_iswt2d.hip).  A detail
// coefficient passes through its plane's operator (BandOp: KEEP, ZERO, SCALE, HARD, SOFT) as it is read.
struct IswtLineArgs {
	const char *src_h, *src_l; // H of level l of line y at src_h + l*plane_stride + y*src_line_stride; the last level's L at src_l + y*src_line_stride
	long plane_stride, src_line_stride;
	int n_lines, N, levels, vec; // dense lines of N <= N1D_MAX floats; vec: 16-byte loads of every source line are aligned
	int op[SWT_MAX_LEVELS];      // per level
	float param[SWT_MAX_LEVELS];
	char *dst; // dense lines
	long dst_line_stride;
};
// every level of every line in ONE launch, the L chain in LDS
hipError_t launch_iswt_lines(Wavelet w, const IswtLineArgs &a, hipStream_t s);
// one level through global memory, one thread per output sample: dense source lines, dst elements d_es bytes apart
struct IswtLevelArgs {
	const char *src_l, *src_h;
	long l_ls, h_ls;
	int n_lines, N, level, op;
	float param;
	char *dst;
	long d_ls, d_es;
};
hipError_t launch_iswt_level(Wavelet w, const IswtLevelArgs &a, hipStream_t s);
// One 2-D level at dilation 1 << level, columns first and then rows (the forward order reversed): Lr from (LL, LH), Hr from
// (HL, HH) along y, the output from (Lr, Hr) along x.  Every plane is W x H, dense elements.
constexpr int ISWT2D_TILE_W = 256;     // the fused kernel's tile: output columns ...
constexpr int ISWT2D_FUSED_LEVELS = 5; // ... and it runs levels 0 .. 4 (dilations 1 .. 16; DESIGN.md s29 on why)
struct Iswt2dLevelArgs {
	const char *ll, *hl, *lh, *hh; // element (x, y) of image b at ll + b*ll_bs + y*ll_sx + 4*x; the details by d_bs, d_sx
	long ll_bs, ll_sx, d_bs, d_sx;
	int W, H, batch, level;
	int op[3]; // of HL, LH, HH
	float param[3];
	char *dst; // element (x, y) of image b at dst + b*dst_bs + y*dst_sx + x*dst_sy
	long dst_bs, dst_sx, dst_sy;
	char *lr, *hr; // the two passes: dense scratch planes, pitch 4*W, image b at + b*H*4*W
};
bool iswt2d_fused_fits(const Iswt2dLevelArgs &a); // dense dst elements, level below ISWT2D_FUSED_LEVELS, a grid the launch can take
hipError_t launch_iswt2d_fused(Wavelet w, const Iswt2dLevelArgs &a, hipStream_t s); // one launch: four planes read once, dst written once
hipError_t launch_iswt2d_cols(Wavelet w, const Iswt2dLevelArgs &a, hipStream_t s);  // ll, hl, lh, hh -> lr, hr; one thread per sample
hipError_t launch_iswt2d_rows(Wavelet w, const Iswt2dLevelArgs &a, hipStream_t s);  // lr, hr -> dst, any dst strides

// Time-frequency planes (dwt_timefreq.hip): every line of a batch correlated with a bank of complex kernels,
//   out(line, bin, t) = sum over the kernel's taps i, ascending, of x[t - center + i] * conj(k[i])   (taps inside [0, N) only),
// from +0, product and sum rounded separately.  The device bank holds the taps already conjugated.
struct TfBin {
	long off;         // first tap of the bin in the bank's tap array
	int size, center; // 0 <= center < size
	int row, pad;     // plane row the bin writes
};
enum TfOut { kTfComplex = 0, kTfAbs = 1, kTfArg = 2 };
struct TfArgs {
	const char *src;     // element t of line y at src + y*src_ls + t*src_es (bytes)
	long src_ls, src_es;
	int n_lines, N;
	int t0, nt;          // the outputs t0 .. t0+nt-1 of every line are computed
	const float2 *taps;  // (re, -im)
	const TfBin *bins;
	const int *order;    // the bins by falling size: the order workgroups take them in
	int n_bins;
	int out;             // TfOut
	char *dst;           // output (y, row, t) at dst + y*plane_stride + row*row_stride + t*dst_es: a float, or (re, im)
	long plane_stride, row_stride, dst_es;
};
// one thread per output, signal and taps read from global memory; any strides that are multiples of 4
hipError_t launch_tf_plain(const TfArgs &a, hipStream_t s);
// dense lines (src_es == 4), finite taps: the signal window in LDS, the taps wave-uniform, 8 outputs per lane
hipError_t launch_tf_tiled(const TfArgs &a, hipStream_t s);
// the plane operators (phase_derivative_s, detect_ridges{1,2,3}_s of src/gabor.c) over n_planes planes: element (y, x) of
// plane p at base + p*ps + y*sx + x*sy (bytes) on both sides.  op 0: phase derivative (param = limit), 1..3: ridges
struct TfPlaneArgs {
	const char *src;
	char *dst;
	long ps, sx, sy;
	int size_x, size_y, n_planes, op;
	float param;
};
hipError_t launch_tf_plane_op(const TfPlaneArgs &a, hipStream_t s);

// the strided gather / scatter (dwt_util_memcpy_stride_s / _i, src/system.c:102-164) on the device: w x h elements of
// `es` (2, 4 or 8) bytes between a dense image (row pitch `pitch`) and one whose element (y, x) lies at y*sx + x*sy; all in BYTES
hipError_t launch_strided_pack(void *dense, long pitch, const void *strided, long sx, long sy, int es, int w, int h, hipStream_t st);
hipError_t launch_strided_unpack(void *strided, long sx, long sy, const void *dense, long pitch, int es, int w, int h, hipStream_t st);

// device-side view helpers: pitch in BYTES, 4-byte elements
hipError_t launch_conv_show(bool is_int, const void *src, void *dst, long pitch, int w, int h, hipStream_t s);
hipError_t launch_compare(bool is_int, const void *p1, const void *p2, long pitch, int w, int h, unsigned *result, hipStream_t s);

// ---- windows of the inverse 2-D transform (dwt_window2d.hip) ----
// One reconstruction level over a REGION: the samples [xa, xb) x [ya, yb) of LL(l-1) -- a frame of W x H samples -- from
// the coefficients under them and a halo of K samples.  The detail bands are read at their Mallat places in the frame
// (`det`: the frame's origin; H halves from column Wd / row Hd on); the LL band from `ll`, whose element (0, 0) is sample
// (ll_y0, ll_x0) of LL(l) (the frame itself with a zero origin, or the region a deeper level left in scratch); the result
// goes to `out`, whose element (0, 0) is sample (ya, xa).  A workgroup owns one tile of 64 x 64 samples of LL(l-1), the
// tiles starting at multiples of 64 of the level's own coordinates.  Pitches and batch strides in ELEMENTS.
constexpr int WINDOW_TILE = 64;
constexpr int WINDOW_GRID_BATCH = 4096; // frames one trip of the kernels' batch loop covers (grid.z)
struct WindowLevelArgs {
	const void *ll;
	long ll_pitch, ll_bs;
	int ll_x0, ll_y0;
	const void *det;
	long det_pitch, det_bs;
	void *out;
	long out_pitch, out_bs;
	int W, H, Wd, Hd;
	int xa, xb, ya, yb;
	int batch;
};
hipError_t launch_window_level(Wavelet w, const WindowLevelArgs &a, hipStream_t s);
// the w x h elements of es bytes at src (of every frame of the batch) -> dst; pitches and batch strides in ELEMENTS
hipError_t launch_window_copy(int es, const void *src, long src_pitch, long src_bs, void *dst, long dst_pitch, long dst_bs, int w, int h,
	int batch, hipStream_t s);

} // namespace dwt
