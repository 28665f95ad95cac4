// dwt_backend.h -- what the backend's translation units share: the device context, workspace and
// staging helpers, the level-pass helpers, the route of a 2-D call as a value (Call2d).  The only per-thread state is
// the context `g` and the error text `g_err`.  Internal to the shared library (hidden visibility).
#pragma once
#include "../../include/libdwt_hip.h"
#include "dwt_kernels.h"

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <array>
#include <condition_variable>
#include <functional>
#include <initializer_list>
#include <map>
#include <mutex>
#include <thread>
#include <unistd.h>
#include <utility>
#include <vector>

namespace dwtb {
using namespace dwt;

// a device scratch buffer of the context
struct Buf {
	void *p = nullptr;
	size_t bytes = 0;
};

struct Ctx {
	bool inited = false;
	int device = 0;
	int want_device = -1; // dwt_hip_set_device: the device this thread's context binds to (-1: environment / 0)
	hipStream_t stream = nullptr;
	char devname[256] = {0};
	// workspace: device scratch, grown on demand (grow), never shrunk, freed by dwt_hip_finish through bufs()
	Buf stage_img; // frame-sized staging image (in-place detour, generic passes)
	Buf ll[2];     // LL ping-pong
	bool ll_external = false; // the caller owns the LL scratch (dwt_hip_set_workspace): never grown, never freed
	// Two general dense device frames.  frame_a holds the staged frame of a host-pointer or strided call (frame_pack /
	// frame_unpack) for the length of that call.  frame_b is the callee's temporary: the staged destination of the 2-D
	// Mallat calls, the line-pass temporaries of the EAW and interleaved levels, the image copy of the fused EAW levels, the
	// plane stacks of the SWT.  The exception: the 3-D drivers take both as their level pools (dwt_hip_alloc_volumes
	// points them into its arena during a trial).
	Buf frame_a, frame_b;
	Buf vol_out;     // dense result volume of an in-place 3-D forward call (fused levels, then copied back)
	Buf vol_host[2]; // device staging of host volumes (struct volume_t entries)
	Buf eaw_w, eaw_ll[2]; // EAW: device weights of a host-pointer call, LL ping-pong of the fused levels
	Buf feat_ws; // feature statistics: records, slab partials, band table, select histograms (dwt_backend_features.hip)
	Buf swt_ws;  // SWT level by level: the L chain's two dense images (dwt_backend_swt.hip); 2-D: the LL chain and the passes' Lr, Hr (dwt_backend_swt2d.hip)
	Buf cond_ws; // row conditioning: per-row medians, extrema, centres, moves, records (dwt_backend_condition.hip)
	Buf band_ws; // band operators: the per-image operator tables of a batch (dwt_backend_bandops.hip)
	Buf nterm_ws; // N-term approximation: ranks, select histograms, records (dwt_backend_nterm.hip)
	Buf half_f32; // float 9/7 on binary16 storage, line-pass route: the binary32 copies of a level's frame (dwt_backend.hip)
	Buf px_pix, px_planes, px_tmp; // pixel front end: the device mirrors of a host call's pixels and planes, the composite entries' plane stack (dwt_backend_pixels.hip)
	Buf wp_ws; // packet trees, cross-check and staged routes: cost tables, trees, totals, the frame the leaves are gathered in (dwt_backend_wp.hip)
	Buf win_ws; // windows of the inverse: the cross-check route's full result, the window kernels' regions between the levels (dwt_backend_window.hip)
	Buf q_coef, q_index, q_planes, q_ws; // quantization: the device mirrors of a host call's coefficients, indices and bit-plane maps; the step tables and the band counters (dwt_backend_quant.hip)
	Buf sp_planes, sp_pos, sp_val, sp_ws; // sparse streams: the device mirrors of a host call's planes, positions and values; the tiles' counts and the mirror of host offsets / counts (dwt_backend_sparse.hip)
	Buf bp_planes, bp_words, bp_off, bp_ws; // bit-plane streams: the device mirrors of a host call's planes, words and offsets; the blocks' sizes (dwt_backend_bitplane.hip)
	Buf lift_ll[2]; // user-defined lifting wavelets: the LL ping-pong of the fused levels (dwt_backend_lifting.hip)
	// every device scratch buffer above: a new one is declared there, listed here, and named nowhere else for freeing
	auto bufs()
	{
		return std::array{&stage_img, &ll[0], &ll[1], &frame_a, &frame_b, &vol_out, &vol_host[0], &vol_host[1], &eaw_w, &eaw_ll[0], &eaw_ll[1], &feat_ws, &swt_ws, &cond_ws, &band_ws, &nterm_ws, &half_f32, &px_pix, &px_planes, &px_tmp, &wp_ws, &q_coef, &q_index, &q_planes, &q_ws, &win_ws, &sp_planes, &sp_pos, &sp_val, &sp_ws, &bp_planes, &bp_words, &bp_off, &bp_ws, &lift_ll[0], &lift_ll[1]};
	}
	hipEvent_t dl_ev[8] = {}; // strip events of the host downloads (dwt_host_xfer.hip), created once
	hipEvent_t switch_ev = nullptr; // dwt_hip_set_stream: orders a newly set stream behind the old one's work
	// host-pointer calls on large images: level 0 band by band while the image is still crossing PCIe (host_forward_pipelined)
	hipStream_t up = nullptr, down = nullptr;
	hipEvent_t pipe_ev[3][16] = {};
	int host_pipeline = 1; // 0: upload, transform, download one after the other
	void *pin = nullptr; // pinned host staging for host-pointer calls with awkward strides (hipHostFree: not a Buf)
	size_t pin_bytes = 0;
	int feat_groups = 0; // workgroups of the feature slab passes (0: the launcher's rule); results do not depend on it
	int tf_tiled = 1;  // time-frequency planes of dense lines through the LDS-tiled kernel (0: one thread per output, the cross-check)
	int cond_fused = -1; // conditioning of dense rows of up to N1D_MAX samples: 1 in one launch, 0 one kernel per operation (the cross-check), -1 by batch size
	int swt2d_fused = 1; // SWT levels of dense device images below SWT2D_FUSED_LEVELS in one launch each (0: a row pass and a column pass, the cross-check)
	int wp_fused = 1; // wavelet packets: lines of up to N1D_MAX samples in one launch, dense device images one launch per level (0: every node through the exact line passes, the cross-check)
	int pixels_wide = 1; // pixel front end: aligned sides move by 16-byte accesses (0: element by element everywhere, the cross-check)
	int quant_wide = 1; // quantization: aligned sides move by 16-byte accesses (0: element by element everywhere, the cross-check)
	int sparse_wide = 1; // sparse streams: aligned planes move by 16-byte accesses (0: element by element everywhere, the cross-check)
	int bitplane_wave = 1; // bit-plane streams: the ballot / LDS kernels (0: one lane per word, the cross-check)
	int lifting_fused = 1; // user-defined lifting wavelets: schemes of reach <= 8 one tile launch per level (0: one launch per step and direction on a dense copy, the cross-check)
	int window_fused = 1; // windows of the inverse: 2 the window kernels wherever they can run, 0 the inverse driver into scratch and a rectangle copy (the cross-check), 1 the kernels where they were measured to win
	int swt_fused = 1; // SWT lines of up to N1D_MAX samples in one launch (0: one launch per level, the cross-check)
	// options
	SweepTuning tune;
	VolTuning vol;
	int force_generic = 0;
	int eaw_two_pass = 0; // EAW: every level as a row pass and a column pass (dwt_backend_eaw.hip), the fused levels' cross-check
	int fma = 0; // opt-in: contract the float 9/7 lifting steps (not bit-identical to libdwt)
	int il_temporal = 0; // set per interleaved call: the forward sweep of level 0 stores its even rows temporal (in place: the copy back reads them)
	int il_inplace_shell = 1; // interleaved in-place calls: level 0 over a snapshot of the tile halos (0: through a staging image, the cross-check)
	int il_exact_borders = 1; // interleaved 9/7: 0 = skip the exact border strips (opt-in: not bit-identical in the top 8 rows / last 5 columns of a level)
	// placement of the LL scratch (DESIGN s5): on the first forward call that needs `place_min_mib` or more of
	// scratch, up to `place_tries` allocations of it -- each behind a spacer that moves it into other
	// physical memory -- are timed with the call's own first two levels and the fastest kept
	// Measurement never happens inside an ordinary transform call (round 5): dwt_hip_tune runs the tile-height
	// tuner and the scratch placement search on the caller's buffers, once, and the context remembers the
	// results; a transform call looks them up, allocates plainly and launches each level once.  DWT_HIP_TUNE=1 in
	// the environment (option "tune_in_call") restores the implicit behaviour for programs that only know libdwt.h.
	int tune_tiles = 1; // use / measure tile heights of large levels (tuned_tile_pairs); 0: the launcher's rule
	std::map<unsigned long long, int> tile_cache;
	int place_tries = 4;  // candidates of the scratch placement search (< 2: no search)
	int place_min_mib = 1024;
	int place_max_gib = 0; // cap of the placement arena of dwt_hip_alloc_batch / _volumes (0: free memory - 8 GiB)
	int tune_in_call = -1; // -1: read DWT_HIP_TUNE on first use
	bool tuning = false;        // inside dwt_hip_tune: measurements allowed
	bool placing = false;       // inside a timed trial: no nested search
	long stat_launches = 0, stat_allocs = 0; // kernel launches / device allocations made by this context's 2-D drivers (tests)
	int stat_choice01 = 0; // the measured choice (apply_tile_choice) the last fused pair of levels 0 and 1 ran with; 0: the launcher's rule (tests)
	int stat_updown01 = 0; // the tile rows that marched upward in that launch (fwd01_updown: 0, 1, 2)
	double place_ms[8] = {0};   // what the last search measured, per candidate
	int place_n = 0, place_best = -1;
	int fused_d = 1; // double-precision wavelets through the fused sweeps (0: exact line passes only)
	int fuse01 = 1;  // forward float 9/7, out of place: levels 0 and 1 in one launch -- 1 where it pays, 2 wherever it can run, 0 never (pair01_ok)
	int fuse_deep = 1; // ... and levels (2, 3), (4, 5) ... of the same calls from scratch, one launch each -- 1 where it pays, 2 wherever it can run, 0 never (pair_deep_ok)
	int stat_deep_pairs = 0; // the pairs below level 1 that the last forward call launched (tests)
	int ride_copy = 1; // in-place calls on one image: the staged subbands' copy rides along with the deeper levels' launches (0: a launch of its own)
	int ride_mib = 32; // ... MiB of it per small level (8192^2: 8 / 16 / 24 / 32 / 48 MiB: forward 202 / 202 / 199 / 199 / 199 us, inverse 224 / 227 / 225 / 224 / 229)
	// profiling
	int prof_on = 0;
	std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
	std::vector<int> prof_tag; // level index of each recorded pair
	size_t prof_used = 0;
	double prof_ms = 0;
	int prof_launches = 0;
	double prof_level_ms[16] = {0};
	int prof_level_n[16] = {0};
};

// One context PER HOST THREAD: its own device binding, stream, workspace and options.  Calls from
// different threads therefore never share scratch buffers (the library is reentrant across
// threads), and one process drives several GPUs with one thread per device: each thread calls
// dwt_hip_set_device(d) first ("single process, 8 devices, one host thread per
// device").  Options set through dwt_hip_set_option / dwt_util_set_accel are per thread too.
extern thread_local Ctx g;
extern thread_local char g_err[512];
// The route of ONE 2-D call as a value: its entry decides it once (call2d) from the wavelet and from the images the
// transform will RUN ON -- the staged ones where the call is staged -- and every driver below takes it as an argument.
// Nothing about a call's route outlives the call.
struct Call2d {
	Wavelet w;
	int es;       // elem_size(w)
	bool aligned; // every base, pitch and batch stride of those images is a multiple of 4 bytes
	// The route rule of the wavelets of 2-byte elements (the int16 5/3, the float 9/7 on binary16 storage): the fused sweeps of
	// dwt_sweep2d_i16.hip / dwt_sweep2d_h.hip take aligned images (a lane's own bytes of a row are then dword-aligned);
	// anything else takes the exact line passes at every level
	bool line_passes_only() const { return es == 2 && !aligned; }
};
Call2d call2d(Wavelet w, std::initializer_list<const void *> ptrs, std::initializer_list<long> strides);
// the wavelet the 32-bit sweeps are launched with (option "fma": the contracted float 9/7)
inline Wavelet sweep32_wavelet(Wavelet w) { return (g.fma && w == kCdf97S) ? kCdf97SFma : w; }

int fail(const char *fmt, ...);
// the tail of a kernel launch that this context counts (stat_launches): 0, or fail("<family> <what> launch failed: ...")
int launched(hipError_t e, const char *family, const char *what);
// device memory is read and written as 4-byte words: every address and stride of a device call is a multiple of 4 bytes
int check_dev_align(std::initializer_list<const void *> ptrs, std::initializer_list<long> strides);
// do na bytes at a and nb bytes at b share a byte?
inline bool overlap(const void *a, size_t na, const void *b, size_t nb)
{
	const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
	return na && nb && pa < pb + nb && pb < pa + na;
}

// The public wavelet id of a C-ABI call (enum dwt_hip_wavelet) as the internal enum Wavelet: the row of kWaveletFacts that
// names it.  false: no such public id (7 is none; the internal wavelets have none).
static_assert(facts(kInterp53S).id == DWT_HIP_INTERP53_S && facts(kCdf53I16).id == DWT_HIP_CDF53_I16 && facts(kCdf97H).id == DWT_HIP_CDF97_H, "kWaveletFacts");
static inline bool wavelet_of(int id, Wavelet *w)
{
	for (int k = 0; id >= 0 && k < kWavelets; k++)
		if (kWaveletFacts[k].id == id) {
			*w = (Wavelet)k;
			return true;
		}
	return false;
}

#define HIP_TRY(expr)                                                                          \
	do {                                                                                       \
		hipError_t e_ = (expr);                                                                \
		if (e_ != hipSuccess)                                                                  \
			return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
	} while (0)

inline int ceil_div_pow2(int i, int j) { return (i + (1 << j) - 1) >> j; } // src/inline.h:455-461
inline int ceil_log2(int x)                                               // src/inline.h:443-448
{
	int n = 0;
	while (n < 31 && (1 << n) < x)
		n++;
	return n;
}
inline long align_up(long v, long a) { return (v + a - 1) / a * a; }

// A device image: element (y,x) at p + y*sx + x*es (dense elements of es = 2, 4 or 8 bytes).
struct Img {
	char *p;
	long sx;    // row pitch in bytes
	int es = 4; // element size in bytes
};

struct Geom {
	int sox, soy, six, siy;
	int Wo(int j) const { return ceil_div_pow2(sox, j); }
	int Ho(int j) const { return ceil_div_pow2(soy, j); }
	int Wi(int j) const { return ceil_div_pow2(six, j); }
	int Hi(int j) const { return ceil_div_pow2(siy, j); }
	bool dense() const { return sox == six && soy == siy; }
};

int grow(Buf &b, size_t need); // at least `need` bytes (never shrinks; a larger buffer replaces the old one behind a stream synchronise)
void dev_free(void *p); // hipFree, or the release of a buffer mapped by dwt_placement.hip
void drop(Buf &b);      // dev_free and forget (the caller has synchronised)
int grant_range(const void *p, int owner, const int *devices, int n_devices); // a placed (VMM) buffer made reachable for these devices; plain allocations: no-op
int copy_rect_on(hipStream_t st, Img dst, long dx, long dy, Img src, long sx_, long sy_, long w, long h);
int copy_rect(Img dst, long dx, long dy, Img src, long sx_, long sy_, long w, long h);
int zero_rect(Img img, long x, long y, long w, long h);
// The staging detour of every driver (dwt_host_xfer.hip).  A frame that cannot run where it lies -- host memory, or a
// device image whose elements are not adjacent or not aligned; each driver keeps its own rule for that -- is packed into
// a dense device image (usually Ctx::frame_a), transformed there and spread back: only the frame's own elements are
// written.  Device frames are packed / spread by a kernel on g.stream (dwt_strided.hip; not counted in stat_launches),
// host frames cross PCIe and those two calls end synchronised (awkward host pitches go through the pinned buffer).
// w x h elements of es bytes, rows sx bytes apart, elements sy bytes apart, in host or device memory
struct Frame {
	void *p;
	long sx, sy;
	int es, w, h;
	bool dev;
};
// host frames take strides below 2 GiB.  The check lives in pack / unpack; a driver calls it itself only where the error
// has to come before it allocates or writes anything (1-D, SWT)
int frame_check(const Frame &f);
int frame_pack(const Frame &f, void *dense, long pitch);         // -> dense device image
int frame_unpack(const Frame &f, const void *dense, long pitch); // dense device image -> the frame's own elements
// the pitch every staged frame takes, and the whole first half of the detour: `buf` grown to f.h rows of that pitch, the
// frame packed into it, *dense describing it
inline long frame_pitch(long es, long w) { return align_up(es * w, 256); }
int frame_stage(const Frame &f, Buf &buf, Img *dense);
// n frames like f, plane_stride bytes apart from f.p on <-> a dense stack of images of `pitch`, pitch * f.h bytes apart
int frame_pack_stack(Frame f, int n, long plane_stride, void *stack, long pitch);
int frame_unpack_stack(Frame f, int n, long plane_stride, const void *stack, long pitch);
int host_volume_xfer(bool to_device, void *dev, size_t d_sy, size_t d_sz, void *host, size_t h_sy, size_t h_sz, int nx, int ny, int nz);
// one exact out-of-place 1-D pass over the lines of a frame (in == out is staged)
int generic_pass(Wavelet w, bool inverse, bool rows, Img in, Img out, int frame_w, int frame_h, int n_lines, int N, int hoff);
// placement (dwt_backend.hip / dwt_placement.hip)
size_t ll_band_bytes(const Geom &ge, int k, int batch, int es); // bytes of LL scratch band k (0: level-1 band, 1: level-2 band)
int timed_forward(const Call2d &c, Img s, Img d, const Geom &ge, int levels, int batch, long sb, long db, double *ms); // ms of the 2nd of two calls
int place_ll_scratch(const Call2d &c, Img s, Img d, const Geom &ge, int levels, int batch, long sb, long db);
int tune2d(const Call2d &c, bool inverse, Img s, Img d, const Geom &ge, int levels, int batch, long sb, long db);
bool stream_is_capturing();
bool may_measure(); // inside dwt_hip_tune, or DWT_HIP_TUNE=1 / option "tune_in_call"
int tuned_tile_pairs(Wavelet w, const FwdLevelArgs &a); // the measured choice for this level (packed; 0: none) ...
int tuned_tile_pairs(Wavelet w, const InvLevelArgs &a);
int tuned_tile_pairs01(Wavelet w, const FwdLevelArgs &a); // the same for the fused pair of levels 0 and 1 (launch_fwd01)
int tuned_updown01(Wavelet w, const FwdLevelArgs &a, const SweepTuning &t); // the measured direction of the fused pair's tile rows under `t` (0, 1; -1: none)
enum TileUse { kTileFwd, kTileInv, kTileFwd01 }; // whose launch a measured choice is for: a forward level, an inverse level, the fused pair
void apply_tile_choice(int choice, SweepTuning *t, TileUse use); // ... applied to the launch's tuning
int forward2d(const Call2d &c, Img src, Img dst, const Geom &ge, int *jp, int decompose_one, int zero_padding, int batch, long src_bstride, long dst_bstride);
int inverse2d(const Call2d &c, Img src, Img dst, const Geom &ge, int j_max, int decompose_one, int zero_padding, int batch, long src_bstride, long dst_bstride);
bool level_fused_ok(const Call2d &c, const Geom &ge, int j); // reads options "generic" and "fused_d" when asked
// the 1-D drivers (dwt_backend_1d.hip): n_lines lines `line_stride` bytes apart, elements `elem_stride` bytes apart, host
// or device; *jp as the reference's forward (clamped, stored) / inverse (read) takes it
int transform1d(Wavelet w, bool inverse, const void *src, void *dst, long line_stride, long elem_stride, int n_lines,
	int so, int si, int *jp, int zero_padding); // level j runs on the fused sweeps (dense frame, both sides >= 2)
// host-pointer calls on large images, band by band under their own PCIe transfers (dwt_host_xfer.hip):
// 0 done, 1 error, -1 not applicable (the caller takes the plain path)
int host_forward_pipelined(const Call2d &c, const void *src, void *dst, int stride_x, int W, int H, int *jp, int decompose_one);
int host_inverse_pipelined(const Call2d &c, const void *src, void *dst, int stride_x, int W, int H, int j_max, int decompose_one);
// the stationary wavelet transform of rows (dwt_backend_swt.hip): device memory on every side, H of level l of line y at
// dst_h + l*plane_stride + y*dls with elements h_es bytes apart, L by l_mode; level l at dilation 1 << (level0 + l)
bool swt_fused_ok(const void *src, long ls, long es, int N);
int swt_device(Wavelet w, const char *src, long ls, long es, int n_lines, int N, int level0, int levels, char *dst_h, long h_es,
	char *dst_l, long l_es, int l_mode, long plane_stride, long dls, int border = kSwtReplicate);
// the warning counters of dwt_hip_rows_warnings lie in cond_ws: forgotten when the scratch is overwritten (dwt_backend_condition.hip)
void cond_forget_warnings();
// the median magnitude of one band of every frame of a batch, the frames only read (dwt_backend_features.hip) -> med (host)
int band_abs_median(const void *ptr, long bstride, int batch, long stride_x, int fw, int fh, int x0, int y0, int w, int h, float *med);
// A side of a call that lies in host or in device memory on its own (the pixel front end, the quantizer): a host side is
// mirrored in a device buffer of the context -- its whole region crosses PCIe -- and a written one crosses back.
struct Side {
	const void *p; // as the caller gave it
	size_t extent; // bytes from p to the end of the last element
	bool dense;    // every byte of the region is an element of the frame
};
// *acc += count * stride, false on overflow
inline bool mul_add(long *acc, long count, long stride)
{
	long t;
	return !__builtin_mul_overflow(count, stride, &t) && !__builtin_add_overflow(*acc, t, acc);
}
inline bool all16(std::initializer_list<uintptr_t> v)
{
	uintptr_t o = 0;
	for (uintptr_t x : v)
		o |= x;
	return o % 16 == 0;
}
// outputs that fit the Infinity Cache with room to spare are stored temporal: what reads them next -- level 0 of the
// transform, the next operator, a copy to the host -- finds them there.  Larger ones would only push each other out
inline int nt_for(size_t out_bytes) { return out_bytes > ((size_t)128 << 20); }
int mirror(const Side &s, Buf &buf, bool upload, char **dev, bool *is_host); // a host side's mirror in `buf`; *dev: where the kernel finds the side
int mirror_back(const Side &s, const Buf &buf);
int prof_drain();
void prof_before(int level = 0);
void prof_after(int level = 0);
int check_inited();

} // namespace dwtb
