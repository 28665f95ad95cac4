/*
 * libdwt_hip.h -- C-ABI of the MI355X (gfx950) backend behind libdwt's 2-D entry
 * points.  Plain C: pointers, ints and sizes only.
 *
 * The functions declared in include/libdwt.h (dwt_cdf97_2f_s & co.) are thin C
 * wrappers over dwt_hip_transform2d(); this header is what a foreign-function
 * binding (cgo, JNI, ctypes ...) or the reference's own sources would bind when they
 * want the device path directly, keep images resident in HBM, run batches, pick a
 * stream or read kernel timings.  See INTEGRATION.md.
 *
 * Pointer rule for every transform entry: `src`/`dst`/`ptr` may be ordinary host
 * memory (any byte strides; staged through HBM, result copied back) or device
 * memory (hipMalloc / dwt_hip_malloc / a torch tensor's data_ptr; transformed in HBM, nothing
 * crosses PCIe).  Device images with adjacent, aligned elements (stride_y == element size, stride_x and
 * the pointer multiples of it) are what the fused sweeps read and write directly.  Any other byte strides
 * -- one channel of an interleaved multi-channel matrix as src/cvdwt.cpp:98-135 passes it (ptr = data +
 * elemSize1*channel, stride_y = elemSize), odd pitches -- are packed into a dense image, transformed and
 * spread back ON THE DEVICE, the device-side dwt_util_memcpy_stride_s / _i (src/system.c:102-164): only
 * the image's own elements are written; rows must not overlap (stride_x >= (width-1)*stride_y + element
 * size).  The batch and 3-D entries take dense rows only.  Every wavelet runs on fused tile sweeps (float, int32 and, since round 2,
 * double); the exact line-pass kernels serve sparse frames, single-line directions and accel 1.
 *
 * Threading: one context PER HOST THREAD (device binding, stream, workspace, options), so
 * calls from different threads never share scratch memory -- unlike the reference, whose 2-D
 * drivers mutate process globals (src/libdwt.c:12839-12862).  One process drives several
 * GPUs with one thread per device: each thread calls dwt_hip_set_device(d) first.  Options
 * (dwt_hip_set_option, dwt_util_set_accel) and dwt_hip_set_stream are per thread as well.
 * Calls are asynchronous for device pointers (stream-ordered on the stream given to
 * dwt_hip_set_stream) and synchronous for host pointers.  A call whose pointers are all device memory
 * still WAITS for its stream where a value has to reach the host first, each said at its entry: the
 * feature entries (dwt_hip_features2d / _2d_batch / _1d_batch, dwt_hip_swt_features1d_batch,
 * dwt_hip_wp_features1d_batch / _2d_batch: the sums are finished on the host) and dwt_hip_rows_condition on
 * its per-operation route (one flag per centring iteration).  An entry that takes a small per-row array in
 * either memory space (info, center, min, max, displ) waits exactly when that array is host memory.  The
 * results that are host memory by definition make their calls wait as well:
 * dwt_hip_universal_threshold_batch always (lambda), dwt_hip_keep_largest_batch / _keep_largest whenever thr or
 * kept is not NULL.  tests/test_hip_streams.py holds every entry to this on a busy stream.
 *
 * Error rule: every int function returns 0 on success and non-zero on failure with
 * a message retrievable by dwt_hip_last_error().  There is NO CPU fallback: without
 * a usable gfx950 device every transform entry fails.
 */
#ifndef LIBDWT_HIP_H
#define LIBDWT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* wavelet/type selectors; the 2-D drivers they replace are cited in libdwt.h */
enum dwt_hip_wavelet {
	DWT_HIP_CDF97_S = 0, /* float CDF 9/7: dwt_cdf97_2f_s / dwt_cdf97_2i_s (src/libdwt.c:12776, 17040) */
	DWT_HIP_CDF53_I = 1, /* int32 CDF 5/3: dwt_cdf53_2f_i / dwt_cdf53_2i_i (src/libdwt.c:16304, 18142) */
	DWT_HIP_CDF53_S = 2, /* float CDF 5/3: dwt_cdf53_2f_s / dwt_cdf53_2i_s (src/libdwt.c:16470, 18296) */
	DWT_HIP_CDF97_D = 3, /* double CDF 9/7: dwt_cdf97_2f_d / dwt_cdf97_2i_d (src/libdwt.c:12451, 16884) */
	DWT_HIP_CDF53_D = 4, /* double CDF 5/3: dwt_cdf53_2f_d / dwt_cdf53_2i_d (src/libdwt.c:12535, 16962) */
	DWT_HIP_CDF97_I = 5, /* int32 fixed-point CDF 9/7: dwt_cdf97_2f_i / dwt_cdf97_2i_i (src/libdwt.c:16387, 18219) */
	/* (7 stays unassigned: earlier releases document it as an unknown id that every entry refuses) */
	DWT_HIP_CDF53_I16 = 8, /* reversible int16 CDF 5/3 in JPEG 2000 order (columns before rows, ITU-T T.800 F.3.2 / F.3.8.1):
	                          dwt_cdf53_2f_i16 / dwt_cdf53_2i_i16; 2-byte elements; dwt_hip_transform2d, _transform2d_batch,
	                          dwt_hip_alloc_batch and dwt_hip_tune only */
	DWT_HIP_CDF97_H = 9, /* float CDF 9/7 on IEEE binary16 storage: dwt_cdf97_2f_h / dwt_cdf97_2i_h; 2-byte elements, binary32
	                        arithmetic, one rounding to nearest even per level; not reversible, no overflow protection
	                        (max|x| * 2^levels must stay below 65504); the same four entries only */
	DWT_HIP_INTERP53_S = 6 /* float interpolating 5/3 (CDF 5/3 predict step, no update): dwt_interp53_2f_s / dwt_interp53_2i_s
	                          (src/libdwt.c:16801, 18457), 1-D dwt_interp53_1f_s / _1i_s (:16166, :15900); not in the
	                          interleaved layout */
};

/* Lifecycle.  dwt_hip_init picks the device from DWT_HIP_DEVICE, else LOCAL_RANK,
 * else 0; it is idempotent.  Replaces the BCE firmware load of dwt_util_init
 * (src/libdwt.c:19158-19181). */
int dwt_hip_init(void);
void dwt_hip_finish(void);
/* Bind the CALLING THREAD's context to a device (0 .. dwt_hip_device_count()-1); a thread that
 * never calls it uses DWT_HIP_DEVICE / LOCAL_RANK / 0.  Rebinding frees the thread's workspace on
 * the old device.  dwt_hip_get_device: the bound device, -1 before the first use. */
int dwt_hip_set_device(int device);
int dwt_hip_get_device(void);
int dwt_hip_device_count(void);
const char *dwt_hip_device_name(void);
const char *dwt_hip_last_error(void);

/* Run on this hipStream_t (NULL = the default stream).  The context's scratch is shared by its streams: a change of
 * stream makes the new one wait (event) for everything the context queued on the old one, so alternating two streams
 * on one thread is safe -- the chains are serialised where they share scratch.  Independent concurrent chains belong
 * to different host threads (one context each).  Streams under capture are not ordered. */
void dwt_hip_set_stream(void *hip_stream);
/* The running-LL scratch of the 2-D Mallat drivers (two bands: the level-1 band, ceil(W/2) x ceil(H/2)
 * elements per image, and the level-2 band) in memory the CALLER owns and places -- the library then
 * neither grows nor frees it (a call that needs more fails).  Two NULLs hand the scratch back to the
 * library.  Per thread, like the rest of the context.
 * The bytes a call needs of band k (k = 0, 1) for a batch of n images of W x H elements of es bytes, exactly:
 *     align_up(ceil(W / 2^(k+1)), 4) * ceil(H / 2^(k+1)) * es * n + 64
 * (rows of the band lie align_up(width, 4) elements apart, images one after the other; 64 bytes of slack behind them).
 * A call that finds either band smaller is refused ("too small") before it writes anything.  The interleaved entries
 * keep their pyramid in the library's own scratch and are refused while the caller owns the bands. */
int dwt_hip_set_workspace(void *band0, size_t bytes0, void *band1, size_t bytes1);
/* The scratch contract.  The content of every scratch buffer of a context -- a caller-owned workspace included -- is
 * UNSPECIFIED on entry to any call and after it, and no result depends on it: every call writes what it reads.
 * dwt_hip_fill_workspace holds the library to that: it stores `word` into every 32-bit word of every scratch buffer the
 * calling thread's context holds at that moment (the caller-owned bands included; the trailing bytes of a buffer whose
 * size is no multiple of 4 take the word's low bytes), on the context's stream, and does not synchronise.  It is a test
 * instrument and an explicit call: nothing in the library calls it.  The one piece of state that outlives a call inside
 * scratch are the counters behind dwt_hip_rows_warnings; after a fill that query answers as before any conditioning
 * call (it fails).  Returns 0, or 1 with dwt_hip_last_error set. */
int dwt_hip_fill_workspace(unsigned word);
void dwt_hip_sync(void);

/* Placement.  The rate of a forward level depends on where in PHYSICAL memory its three streams lie
 * relative to each other (source rows, detail subbands, running LL band: DESIGN.md s5,
 * profiles/r04_placement.md).  The reference hands its callers a placement-aware allocator for the same
 * kind of reason -- dwt_util_get_opt_stride / dwt_util_get_stride, src/libdwt.c:20641-20707 -- and so does
 * this library:
 *   - the library's own LL scratch: dwt_hip_tune (below) on a forward call (batch or single image, distinct
 *     source and destination, two levels or more) that needs "place_min_mib" (option, default 1024) MiB or more
 *     of it tries up to "place_tries" (option, default 4; 1 = off) allocations, times the call itself on each
 *     and keeps the fastest.  dwt_hip_placement_report returns what the last search measured (ms per
 *     candidate, return value = number of candidates, 0 = no search ran).  A transform call itself never
 *     searches (unless DWT_HIP_TUNE=1): it allocates what it needs once and afterwards nothing.
 *   - dwt_hip_alloc_batch: source and destination of a resident batch of `n_images` dense size_x x size_y
 *     images (pitch size_x elements, images size_x * size_y elements apart) together with the scratch, placed
 *     by measurement: most of the card's free memory is mapped as one arena, the destination is tried at
 *     every 4 GiB step of it (one level against the source), the scratch at every step for the best
 *     destinations (the `levels`-level forward transform of the whole batch; < 0: full depth), the best
 *     arrangement is kept and the rest of the arena returned.  Seconds, once, for a batch that stays
 *     resident; dwt_hip_alloc_batch_report says what was measured.  Free both with dwt_hip_free. */
int dwt_hip_alloc_batch(int wavelet, int n_images, int size_x, int size_y, int levels, void **src, void **dst);
/* the same for the two dense volumes of an out-of-place 3-D call (dwt_hip_transform3d_op) of `levels` levels */
int dwt_hip_alloc_volumes(int size_x, int size_y, int size_z, int levels, void **src, void **dst);
int dwt_hip_placement_report(double *ms, int n);
/* "" when the last dwt_hip_alloc_batch / _volumes of this thread ran its search, else why it allocated plainly */
const char *dwt_hip_alloc_batch_note(void);
/* Buffers of dwt_hip_alloc_batch / _volumes are mapped through the virtual-memory API with access for their owner
 * alone (hipDeviceEnablePeerAccess does not cover such ranges).  dwt_hip_transform2d_batch_sharded grants its
 * slots' devices by itself; dwt_hip_grant_access does it for a caller's own peer copies (`dev_ptr` may point
 * anywhere into the buffer) and, for plain allocations, enables peer access from each device named.
 * 0 = every device named can reach the buffer. */
int dwt_hip_grant_access(void *dev_ptr, const int *devices, int n_devices);
/* MEASUREMENT IS EXPLICIT (round 5).  A transform call never measures anything: it allocates its scratch plainly,
 * launches every level once and uses the launcher's tile rule -- unless dwt_hip_tune has run for its shape on
 * the calling thread's context.  dwt_hip_tune runs the `levels`-level transform on THE CALLER'S OWN BUFFERS
 * (`dst` receives the transform of `src`, as after a call; src != dst, device pointers, batch_stride may be 0
 * for one image) a few times: the scratch placement search (forward, two levels or more, "place_min_mib" MiB of
 * scratch or more: up to "place_tries" allocations behind growing spacers, each timed with the call itself,
 * the fastest kept) and the tile-height tuner (every level whose input is 512 MiB or more -- a level that fits the
 * 256 MiB Infinity Cache cannot be measured by repeating it: 64 / 32 / 16 row pairs forward, 32 / 16 / 8 inverse).  Synchronous, one at a time per device; results are kept by the calling thread's
 * context per (wavelet, direction, width, height, batch) until dwt_hip_finish.  Same bits with and without.
 * The reference's analogue is explicit too: dwt_util_get_opt_stride, src/libdwt.c:20641-20707.
 * Programs that only know libdwt.h: DWT_HIP_TUNE=1 in the environment (option "tune_in_call") lets the first
 * large call of a shape measure by itself, as rounds 3-4 did. */
int dwt_hip_tune(int wavelet, int inverse, const void *src, void *dst, size_t batch_stride, int batch,
	int stride_x, int size_x, int size_y, int levels);
void dwt_hip_alloc_batch_report(int *chunks, int *dst_tried, int *ll_tried, int *dst_at, int *ll_at, double *ms4, double *seconds);

/* Tuning / variant selection (mirrors dwt_util_set_accel, src/libdwt.c:19946).  Every setting gives the
 * same bits; what is left after round 4's pruning is what the tests use as cross-checks or a caller may need.
 * 2-D: "generic" (1 = force the exact line-pass kernels), "cpt" (0 = auto / 4 / 8 columns per lane),
 * "tile_pairs" (0 = auto), "waves" (1..4 per workgroup), "xcd_swizzle" (0/1), "ring" (0 = auto / 8 / 16 LDS
 * rows per wave, forward) and "ring_inv" (8 / 16), "nt" (7 = default cache policy, 3 = the LL band's stores
 * non-temporal too, 15 = 7 with the neighbour taps by wavefront shifts instead of LDS reads), "nt_auto"
 * (1 = policy 3 by itself when a launch's LL bands exceed 1 GiB), "fma" (1 = contracted lifting steps:
 * NOT the reference's rounding, within 1e-5), "fused_d" (0 = double precision through the exact line passes),
 * "fuse01" (forward float 9/7, Mallat, out of place, two levels or more, width and height multiples of 4 with both
 * levels of 64 x 64 or more: levels 0 and 1 in ONE launch, level 0's LL band never written --
 * 1 = where that pays (launches of 32768 tiles of 512 columns x 64 row pairs and more: 32 images of 8192^2, 128 of 4096^2), 0 = never, 2 = wherever
 * the geometry is legal, for tests; same bits; not with "fma", "cpt" 4, "ring" 8, "nt" 15 or an odd "tile_pairs"),
 * "fuse_deep" (the same launch for levels 2 and 3, 4 and 5 ... of such a call, each pair from one LL scratch band to the other:
 * 1 = where that pays -- in calls whose levels 0 and 1 ran in one launch by the size rule above, in launches of 2048 tiles of
 * 512 columns x 64 row pairs and more (level 2 of 32 images of 8192^2), then with the 8-row ring, the odd tile rows upward and
 * 128 row pairs unless set by hand or measured by dwt_hip_tune --, 0 = never, 2 = wherever the geometry of the pair's first
 * level is legal, for tests; same bits, the same workspace; dwt_hip_get_option("fuse_deep_last") reads how many such pairs the
 * last forward call launched),
 * "fuse01_ring" (the LDS ring rows per wave of that one launch: 16 = one workgroup of four waves per CU, 8 = two of them, two
 * waves per SIMD; 0 = the launcher's rule -- 8 from 32768 tiles on, else 16 -- or what dwt_hip_tune measured; any other value is
 * refused; same bits),
 * "fuse01_updown" (which tile rows of that launch march from their lower edge upward, so that vertically adjacent tiles read
 * the rows around their common edge at the same time and the second read hits in L2: 0 = none, 1 = the odd ones, 2 = the even
 * ones (for tests), -1 = the launcher's rule -- 1 in launches of 32768 tiles and more that run the 8-row ring, whether the ring's rule or
 * "fuse01_ring" chose it, else 0 -- or what dwt_hip_tune measured;
 * any other value is refused; same bits; dwt_hip_get_option("fuse01_last_updown") reads what the last such launch ran with),
 * "ride_copy" (1 = in-place Mallat calls on one image: the copy of level 0's staged subbands rides along with the deeper
 * levels' launches as extra workgroups; 0 = a launch of its own, the cross-check) and "ride_mib" (MiB of it per small level),
 * "host_pipeline" (1 = host-pointer calls on images of 64 MiB and more run band by band under their own
 * PCIe transfers, the caller's memory pinned in place for the call; 0 = upload, transform, download),
 * "il_inplace_shell" (1 = in-place calls of the interleaved entries run level 0 in place over a snapshot of the tile
 * halos; 0 = through a staging copy of the image, the cross-check),
 * "il_exact_borders" (0 = no border strips at all: the top 8 rows / last 5 columns of a level keep the sweep's
 * rows-then-columns rounding -- NOT the reference's bits there, a few ulp, far inside 1e-5; opt-in like "fma"),
 * "tune_tiles" (1 = levels of 512 MiB and more use the tile height dwt_hip_tune measured for their shape;
 * 0 = always the launcher's rule), "tune_in_call" (1 = the first large call of a shape measures by itself;
 * default: DWT_HIP_TUNE), "place_tries" / "place_min_mib" (placement search, below), "place_max_gib" (cap of the
 * arena dwt_hip_alloc_batch / _volumes map for their search; 0 = free memory - 8 GiB).
 * Read-only: "stat_launches" / "stat_allocs" (kernel launches / device allocations of this context's 2-D drivers
 * so far), "tile_cache_size", "place_last_tries", "place_last_best", "fuse01_last_choice", "fuse01_last_updown",
 * "fuse_deep_last".
 * 3-D: "vol_fused" (1 = one-pass levels where they pay, 2 = wherever they can run, 0 = two passes),
 * "vol_whole" (0 = the general kernel variant as a cross-check), "vol_direct" (levels >= 1 into their lattice
 * of the destination: 2 = rows shared by levels 0 and 1 written once, 1 = sample-wise stores, 0 = dense
 * results + scatter passes), "vol_nt", "vol_rows" (8 / 6), "vol_tile_pairs", "vol_swizzle",
 * "vol_ip_waves" (0 = auto / 4 / 8 waves per workgroup of the one-pass levels: tiles of 32 or 64 rows),
 * "vol_inplace_fused" (in-place calls: 1 = one fused pass per level in place over a snapshot of the tile
 * halos, forward and inverse; 0 = two passes per level).
 * Environment (diagnostics only, read once): DWT_HIP_PLACE_VERBOSE (the placement search prints its timings),
 * DWT_HIP_TUNE_VERBOSE (the tile tuner prints every candidate's time),
 * DWT_HIP_PIPE_VERBOSE (a pipelined host-pointer call prints when its upload / download streams end),
 * DWT_HIP_PIPE_BAND (row pairs per band of such a call, a multiple of 64; default 256). */
int dwt_hip_set_option(const char *name, int value);
int dwt_hip_get_option(const char *name);

/* Multi-level 2-D transform, Mallat layout, all arguments as in libdwt's drivers
 * (src/libdwt.h:562-573, 867-878, 667-679, 962-974).  src == dst selects the
 * in-place entries, src != dst the `_s2` out-of-place entries.  `*j` is in/out for
 * forward (clamped as the reference does) and in for inverse. */
int dwt_hip_transform2d(int wavelet, int inverse, const void *src, void *dst,
	int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int *j, int decompose_one, int zero_padding);

/* Multi-level 1-D transform of one float line (wavelet DWT_HIP_CDF97_S,
 * DWT_HIP_CDF53_S or DWT_HIP_INTERP53_S), Mallat layout, arguments as in libdwt's 1-D drivers
 * (src/libdwt.h:1128-1208): elements `stride` bytes apart, `*j` in/out for forward
 * (clamped as the reference does), in for inverse.  src == dst: in place; otherwise
 * dst receives the transform of src's frame.  Host or device pointers (host: the call
 * is synchronous; device: ordered on the context's stream). */
int dwt_hip_transform1d(int wavelet, int inverse, const void *src, void *dst,
	int stride, int size_o, int size_i, int *j, int zero_padding);

/* The same on `n_lines` lines `line_stride` bytes apart, elements `elem_stride` bytes
 * apart (one channel of interleaved data: elem_stride = channels * 4).  Dense lines of
 * up to 8192 samples run all levels in one kernel launch. */
int dwt_hip_transform1d_batch(int wavelet, int inverse, const void *src, void *dst,
	size_t line_stride, int elem_stride, int n_lines, int size_o, int size_i, int *j, int zero_padding);

/* Edge-avoiding CDF 5/3 wavelets (EAW, Fattal 2009; libdwt's dwt_eaw53_*: src/libdwt.h:742-796, 1073-1100), float.
 * layout DWT_HIP_EAW_MALLAT: dwt_eaw53_2f_s / _2i_s; DWT_HIP_EAW_INTERLEAVED: dwt_eaw53_2f_inplace_s / _2i_inplace_s.
 * In place on `ptr` (host or device memory, any byte strides); `*j` in/out for forward (clamped as the reference
 * does), in for inverse.  `weights` is ONE caller-owned buffer in the same memory space as `ptr`, laid out as
 * dwt_hip_eaw53_weights_layout says for the call's level count: the forward writes every level's wH / wV there (the
 * reference's shapes and orders; entries of one-sample lines are left as they were), the inverse reads them.  alpha 1
 * and 0 give the reference's bits; any other alpha computes |d|^alpha in double rounded once to float (within 1 ulp
 * of glibc's powf).  The inverse is exact for every alpha.  A dense Mallat frame in HBM runs one launch per level. */
#define DWT_HIP_EAW_MALLAT 0
#define DWT_HIP_EAW_INTERLEAVED 1
int dwt_hip_eaw53_2d(int inverse, int layout, void *ptr, int stride_x, int stride_y, int size_o_x, int size_o_y,
	int size_i_x, int size_i_y, int *j, int decompose_one, int zero_padding, float *weights, float alpha);

/* The same on `batch` dense Mallat images in HBM (size_o == size_i), `batch_stride` bytes apart, zero_padding 0;
 * image b's weights at weights + b * weights_stride floats.  One launch per level covers the whole batch. */
int dwt_hip_eaw53_2d_batch(int inverse, void *ptr, size_t batch_stride, int batch, int stride_x, int size_x, int size_y,
	int *j, int decompose_one, float *weights, size_t weights_stride, float alpha);

/* Edge-avoiding CDF 9/7 wavelet (libdwt's dwt_eaw97_2f_s / _2i_s, "WCDF 9/7": src/eaw-experimental.h), float, Mallat
 * layout only (the reference has no interleaved twin).  Four lifting steps per pass, all with the weights computed once
 * from the pass's input.  The contracts are those of dwt_hip_eaw53_2d / _batch above: host or device memory, any byte
 * strides, one caller-owned weight buffer in the memory space of `ptr`, alpha 1 and 0 exact, any other alpha through
 * pow in double, the inverse exact for every alpha, one launch per level of a dense Mallat frame in HBM.  The weight
 * arrays have the shapes of the 5/3 wavelet's, so dwt_hip_eaw53_weights_layout(DWT_HIP_EAW_MALLAT, ...) lays out the
 * buffer of both wavelets. */
int dwt_hip_eaw97_2d(int inverse, void *ptr, int stride_x, int stride_y, int size_o_x, int size_o_y, int size_i_x,
	int size_i_y, int *j, int decompose_one, int zero_padding, float *weights, float alpha);
int dwt_hip_eaw97_2d_batch(int inverse, void *ptr, size_t batch_stride, int batch, int stride_x, int size_x, int size_y,
	int *j, int decompose_one, float *weights, size_t weights_stride, float alpha);

/* Floats of the weight buffer of a `j`-level EAW call, 5/3 or 9/7 (-1: bad arguments); off_h[k] / off_v[k] (k < j; either
 * may be NULL) receive where level k's wH / wV start.  Mallat: wH[k] is size_o_src_y x size_i_src_x row-major, wV[k]
 * size_o_src_x x size_i_src_y column-major (wV[k][x * size_i_src_y + y]); interleaved: both size_i_src_y x size_i_src_x
 * (wV column-major too). */
long dwt_hip_eaw53_weights_layout(int layout, int size_o_x, int size_o_y, int size_i_x, int size_i_y, int j,
	long *off_h, long *off_v);

/* Batch of independent equally sized dense images resident in HBM, `batch_stride`
 * bytes apart; one launch per level covers the whole batch.  Addresses and strides are multiples of the element
 * size (this entry has no staging detour: anything else is refused). */
int dwt_hip_transform2d_batch(int wavelet, int inverse, const void *src, void *dst,
	size_t batch_stride, int batch, int stride_x, int size_x, int size_y, int *j);

/* The same batch sharded over several GPUs of ONE process (images are independent: no
 * collective in the transform).  `src` / `dst` lie in the memory of the calling thread's device, which must
 * be devices[0]; image b belongs to slot b * n_slots / batch (n_slots = min(n_devices, batch)), i.e. slot k
 * owns the images [ceil(k * batch / n_slots), ceil((k + 1) * batch / n_slots)) -- dwt_hip_shard_bounds.
 * Slot 0's shard is transformed where it lies; every other slot is a persistent host thread with its own
 * context on devices[k] (a device may be named more than once) that pulls its shard across
 * (hipMemcpyPeerAsync over xGMI) in up to four pieces, transforms each with dwt_hip_transform2d_batch and
 * pushes the result back while the next piece arrives -- all slots at the same time.  Synchronous: returns
 * when `dst` is complete.  Bytes of `dst` outside the frames keep their values.  Root-egress bound: the
 * whole batch leaves and re-enters one device. */
int dwt_hip_transform2d_batch_sharded(int wavelet, int inverse, const void *src, void *dst,
	size_t batch_stride, int batch, int stride_x, int size_x, int size_y, int *j, const int *devices, int n_devices);
/* slot outside [0, n_slots) or batch < 0: *count = 0 */
void dwt_hip_shard_bounds(int batch, int n_slots, int slot, int *first, int *count);

/* The batch split for shards that are RESIDENT where they are transformed ("the >= 7x scaling
 * claim is measured on per-GPU-resident data"): shard k -- counts[k] images at srcs[k] / dsts[k],
 * `batch_stride` bytes apart -- lies in the memory of devices[k] (allocated there by a thread bound to it with
 * dwt_hip_set_device; a device may be named more than once; counts[k] == 0 skips a shard).  All shards are
 * transformed at the same time, each by a persistent host thread with a context of its own on its device (the
 * calling thread takes the first shard on its own device); nothing crosses xGMI.  Synchronous; every shard's device is
 * drained (hipDeviceSynchronize) before its shard is read, so producers on any stream of that device come first.  `*j` as in
 * dwt_hip_transform2d_batch.  dwt_hip_tune_batch_multi runs dwt_hip_tune in every slot instead (once, before
 * the first transform of shards that stay resident): the slots' contexts keep what it measures. */
int dwt_hip_transform2d_batch_multi(int wavelet, int inverse, const void *const *srcs, void *const *dsts, const int *counts,
	const int *devices, int n_shards, size_t batch_stride, int stride_x, int size_x, int size_y, int *j);
int dwt_hip_tune_batch_multi(int wavelet, int inverse, const void *const *srcs, void *const *dsts, const int *counts,
	const int *devices, int n_shards, size_t batch_stride, int stride_x, int size_x, int size_y, int levels);

/* 2-D transforms in the INTERLEAVED (in-place lifting) layout: no de-interleave, level j
 * works on the stride-2^j lattice of the image (even lattice index = low-pass).
 * `wavelet` is DWT_HIP_CDF97_S or DWT_HIP_CDF53_S (and, flavour 0 only, DWT_HIP_CDF97_I for
 * dwt_cdf97_2f_inplace_i / dwt_cdf97_2i_inplace_i, src/libdwt.c:17424, 17308).  `flavour` 0 = libdwt.h's
 * dwt_cdf97_2f_inplace_s / dwt_cdf97_2i_inplace_s / dwt_cdf53_2f_inplace_s /
 * dwt_cdf53_2i_inplace_s (src/libdwt.c:12926, 17474, 16553, 17886); flavour 1 =
 * dwt-simple.h's forward fdwt2_cdf97_* / fdwt2_cdf53_* (src/dwt-simple.c:2224, 2356); flavours
 * 2 / 3 = fdwt2h1_cdf97_vertical_s / fdwt2v1_cdf97_vertical_s (rows only / columns only, :1747, :1837).
 * Host or device pointers, in place (src == dst) or out of place. */
int dwt_hip_transform2d_interleaved(int wavelet, int inverse, int flavour, const void *src, void *dst,
	int stride_x, int stride_y, int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int *j, int decompose_one);

/* Single-level 3-D CDF 9/7 float over the interleaved in-place layout of
 * cdf97_3f_ip_sep_horizontal_s / cdf97_3i_ip_sep_horizontal_s
 * (src/volume-dwt.c:677, 1115); `levels` > 1 re-applies it on the LLL lattice
 * (strides doubled) as SURVEY.md s8 a11 describes.  Device pointer, dense x.  Levels of 512^3 and
 * more (256 tiles of 256 x 64 voxel columns or more) run in ONE pass in place (tile halos read from a
 * snapshot, ~10.8 B per voxel), smaller ones in two passes through a scratch volume.  The volume's address and
 * both strides are multiples of 4 bytes, in this entry, in dwt_hip_transform3d_op and for the device volumes of the
 * struct volume_t entries below: anything else is refused with a message and nothing is written. */
int dwt_hip_transform3d(int inverse, void *vol, size_t stride_y, size_t stride_z,
	int size_x, int size_y, int size_z, int levels);

/* The same forward transform OUT OF PLACE (src != dst, both device pointers, same strides):
 * cdf97_3f_op_sep_horizontal_s (src/volume-dwt.c:727-785), the entry the reference's 3-D
 * perf test drives.  Each level is one fused x+y+z pass where that pays (volumes of about
 * 448^3 and more, at least 128 samples wide; any size and 4-byte alignment), two passes otherwise. */
int dwt_hip_transform3d_op(const void *src, void *dst, size_t stride_y, size_t stride_z,
	int size_x, int size_y, int size_z, int levels);

/* The same two transforms on the FIELDS of the reference's struct volume_t (include/volume.h; the
 * typed wrappers cdf97_3f_op_sep_horizontal_s & co. of include/volume-dwt.h sit on these): one level,
 * host or device pointers (host volumes are staged through HBM), source and destination with
 * their own row / slice strides in bytes, samples dense along x.  dirs: 7 = x, y and z; 1 = x lines
 * only (copy, then lift); 2 / 4 = y / z lines only, in place on dst (src unused) -- the reference's
 * VOL_SEP_HORIZONTAL_X / _Y / _Z measurements (src/volume-dwt.c:788, :852, :918). */
int dwt_hip_volume_fwd_op(const void *src, size_t src_stride_y, size_t src_stride_z, void *dst, size_t dst_stride_y,
	size_t dst_stride_z, int size_x, int size_y, int size_z, int dirs);
int dwt_hip_volume_ip(int inverse, void *data, size_t stride_y, size_t stride_z, int size_x, int size_y, int size_z);

/* Device-side twins of dwt_util_conv_show_{s,i} (src/libdwt.c:21075, 21020) and
 * dwt_util_compare_{s,i} (:1593, :1531) for images that stay in HBM between a forward and
 * an inverse transform.  compare returns 0 equal / 1 differ (float: 1e-3 absolute, NaN or
 * Inf => differ) / -1 error. */
int dwt_hip_conv_show(int is_int, const void *src, void *dst, int stride_x, int stride_y, int size_x, int size_y);
int dwt_hip_compare(int is_int, const void *ptr1, const void *ptr2, int stride_x, int stride_y, int size_x, int size_y);

/* Device memory helpers so that C callers need no HIP headers. */
void *dwt_hip_malloc(size_t bytes);
void dwt_hip_free(void *dev_ptr);
/* page-locked host memory (what volume_alloc_realiably_locked hands out): DMA without a bounce buffer */
void *dwt_hip_malloc_host(size_t bytes);
void dwt_hip_free_host(void *host_ptr);
int dwt_hip_memcpy_h2d(void *dev_dst, const void *host_src, size_t bytes);
int dwt_hip_memcpy_d2h(void *host_dst, const void *dev_src, size_t bytes);
int dwt_hip_is_device_pointer(const void *p);

/* Per-subband feature statistics of a transformed image (libdwt's dwt_util_wps_s, _maxidx_s, _mean_s, _med_s, _var_s,
 * _stdev_s, _skew_s, _kurt_s, _maxnorm_s, _lpnorm_s, _norm_s: src/libdwt.h:2875-3309), reduced where the coefficients lie.
 * The bands are those of dwt_util_subband for levels 1 .. j_max-1 (level j_max itself is not visited, as in the
 * reference), HL, LH, HH within a level, empty bands skipped: dwt_hip_count_subbands of them.
 * `fv` receives one block of that many floats per feature of the mask, in enum order.  It lies in the memory space of
 * `ptr` (both host or both device); device calls are ordered on the context's stream and wait for it: the raw sums
 * come back to the host, are finished there and go out to `fv` before the call returns.
 * Numerics: maxnorm, maxidx and med are the reference's values for every NaN-free input (med as a value: which of +0 /
 * -0 stands in the middle of equal zeros is unspecified; behaviour on NaN inputs is not pinned, the reference's
 * qsort comparator being no order there).  Sums accumulate in double in a fixed order -- the same bits on every run
 * and for every launch geometry -- are rounded to float once and finished on the host in float as the reference
 * writes it; x - mean is the float subtraction of the float mean.  `p` (> 0, INFINITY allowed) is read by LPNORM only. */
enum dwt_hip_feature {
	DWT_HIP_FEATURE_WPS = 0,
	DWT_HIP_FEATURE_MAXIDX,
	DWT_HIP_FEATURE_MEAN,
	DWT_HIP_FEATURE_MED,
	DWT_HIP_FEATURE_VAR,
	DWT_HIP_FEATURE_STDEV,
	DWT_HIP_FEATURE_SKEW,
	DWT_HIP_FEATURE_KURT,
	DWT_HIP_FEATURE_MAXNORM,
	DWT_HIP_FEATURE_LPNORM,
	DWT_HIP_FEATURE_NORM,
	DWT_HIP_FEATURE_COUNT
};
#define DWT_HIP_FEATURE_BIT(f) (1u << (f))
/* number of non-empty detail bands of levels 1 .. j_max-1; -1 for bad sizes */
int dwt_hip_count_subbands(int size_o_x, int size_o_y, int size_i_x, int size_i_y, int j_max);
int dwt_hip_features2d(unsigned feature_mask, const void *ptr, int stride_x, int stride_y, int size_o_x, int size_o_y,
	int size_i_x, int size_i_y, int j_max, float p, float *fv);
/* the same with `fv` in HOST memory wherever `ptr` lies (what libdwt's dwt_util_*_s entries take) */
int dwt_hip_features2d_hostfv(unsigned feature_mask, const void *ptr, int stride_x, int stride_y, int size_o_x, int size_o_y,
	int size_i_x, int size_i_y, int j_max, float p, float *fv);
/* The raw double sums behind the calling thread's last feature call, for checks of the accumulation: plane 0 sum x,
 * 1 sum x^2, 2 sum |x|^p (p other than 2), 3 .. 5 sum (x - mean)^2, ^3, ^4; one double per (image, band) in call
 * order.  Returns the number copied (at most n), -1 when the last call's mask did not need that plane. */
long dwt_hip_features_raw_sums(int plane, double *out, long n);
/* `batch` dense images batch_stride bytes apart; the vector of image b at fv + b*fv_stride floats */
int dwt_hip_features2d_batch(unsigned feature_mask, const void *ptr, size_t batch_stride, int batch, int stride_x,
	int size_x, int size_y, int j_max, float p, float *fv, size_t fv_stride);
/* n_lines rows of `size` samples (each a frame with size_y = 1), strides in bytes; rows of up to 8192 samples take
 * ONE kernel launch for every band and every feature */
int dwt_hip_features1d_batch(unsigned feature_mask, const void *ptr, size_t line_stride, size_t elem_stride, int n_lines,
	int size, int j_max, float p, float *fv, size_t fv_stride);
/* one statistic of one band (the dwt_util_band_*_s primitives): size_x x size_y elements at ptr (host or device);
 * `j` is read by WPS, `p` by LPNORM; *value is host memory */
int dwt_hip_band_feature(int feature, const void *ptr, int stride_x, int stride_y, int size_x, int size_y, int j, float p,
	float *value);
/* sum powf(x - c, n) / size (dwt_util_band_moment_s); central != 0: about the band's float mean (_cmoment_s) */
int dwt_hip_band_moment(const void *ptr, int stride_x, int stride_y, int size_x, int size_y, int n, int central, float c,
	float *value);
/* |x| in place (dwt_util_abs_s): the sign bit cleared, so -0 -> +0 and Inf stays Inf */
int dwt_hip_abs(void *ptr, int stride_x, int stride_y, int size_x, int size_y);

/* Conditioning of row batches before a transform, as the reference's spectra programs do (dwt_util_shift21_med_s,
 * dwt_util_center21_s, dwt_util_scale21_s, src/libdwt.c:25426-26055).  Sample i of row y lies at
 * ptr + y*line_stride + i*elem_stride (bytes), in host or device memory; rows are conditioned in place.  Dense device
 * rows of up to 8192 samples take ONE launch whatever the iteration count, up to the batch size from which one kernel per
 * operation is faster (option "cond_fused" = 1 / 0 forces either route, -1 restores the choice; same bits).  The per-row arrays (info, center, min, max, displ) may each be host
 * or device memory.  The one-launch route with `info` NULL or in device memory does not wait for the device; the
 * per-operation route with CENTER reads one flag back after every centring iteration and so waits for its stream.
 *   MED_SHIFT  x += -median, the median being the element of rank size/2 of the row's signed values;
 *   CENTER     up to max_iters times: c = the row's centre; stop if c == size/2, else row[x] = row[x + c - size/2] with
 *              zeros moving in (samples moved out are lost: the iterations are not one shift of the original row);
 *   SCALE      x += (lo - min), then x *= ((hi - lo) / (max - min)); a row with max == min is left alone.
 * Everything but the centre decision is the reference's arithmetic bit for bit (NaN-free input).  The centre is decided
 * in float sums in index order like the reference's, over terms |x|^10 formed as double products rounded to float once,
 * where the reference calls powf: rows where a 1-ulp term difference flips a strict comparison can centre differently. */
enum dwt_hip_rows_op { DWT_HIP_ROWS_MED_SHIFT = 1, DWT_HIP_ROWS_CENTER = 2, DWT_HIP_ROWS_SCALE = 4 };
/* ops applied in this order; info (optional): 4 ints per row =
 * { net offset d (out[x] = in[x+d] where kept), moves made, last centre found (-1: none looked for), 1 if SCALE skipped the row } */
int dwt_hip_rows_condition(unsigned ops, void *ptr, size_t line_stride, size_t elem_stride, int n_lines, int size, int max_iters,
	float lo, float hi, int *info);
/* dwt_util_get_center1_s of every row */
int dwt_hip_rows_center_index(const void *ptr, size_t line_stride, size_t elem_stride, int n_lines, int size, int *center);
/* What the reference would have warned about in the centre evaluations of this thread's last dwt_hip_rows_condition or
 * dwt_hip_rows_center_index call: how many found a zero norm, how many found no crossing index (each optional).  The
 * counters lie in scratch: after dwt_hip_fill_workspace the query fails as it does before any such call. */
int dwt_hip_rows_warnings(int *zero_norm, int *no_index);
/* dwt_util_find_min_max_s of every row (as values: which of +0 / -0 stands for an extreme zero is unspecified) */
int dwt_hip_rows_min_max(const void *ptr, size_t line_stride, size_t elem_stride, int n_lines, int size, float *min, float *max);
/* row[x] = row[x + d], d = displ[row] or displ_all; from outside the row comes zero (zero_fill: dwt_util_displace1_zero_s)
 * or the nearest sample (dwt_util_displace1_s) */
int dwt_hip_rows_displace(void *ptr, size_t line_stride, size_t elem_stride, int n_lines, int size, const int *displ, int displ_all,
	int zero_fill);
/* x += a / x *= a over size_x x size_y elements, element (y, x) at ptr + y*stride_x + x*stride_y (dwt_util_shift_s, _scale_s) */
int dwt_hip_shift(void *ptr, int stride_x, int stride_y, int size_x, int size_y, float a);
int dwt_hip_scale(void *ptr, int stride_x, int stride_y, int size_x, int size_y, float a);

/* Per-band coefficient operators: what the reference's synthesis programs do between a forward and an inverse transform
 * (examples/hdr, examples/mra, examples/displ-vectors, src/denoise.c), on coefficients that stay where they lie (DESIGN.md
 * s17).  A Mallat frame decomposed to J levels has 3J + 1 SLOTS: slot 3(j-1) + {0, 1, 2} is HL, LH, HH of level j = 1 .. J,
 * slot 3J is LL of level J, each with the geometry of dwt_util_subband_s over the outer and inner sizes.  Empty bands keep
 * their slot; a frame of one row has its H bands in the HL slots.  Every slot carries one operator and one float `a`:
 *   KEEP      untouched: neither read nor written
 *   ZERO      +0.0f
 *   SCALE     c * a                                   (dwt_util_scale_s)
 *   HARD      fabsf(c) > a ? c : +0.0f
 *   SOFT      c > a ? c - a : (c < -a ? c + a : +0.0f)
 *   COMPRESS  s * P, s = c > 0 ? +1 : -1, P = |c|^a  (dwt_util_compress_s of examples/hdr/hdr.c; P is pow in double
 *             rounded to float once: within 1 ulp of the correctly rounded float, where the reference calls powf)
 * A NaN coefficient is left as it is by every operator but ZERO.  ONE kernel launch applies the whole table to every
 * frame of a batch, in place; a table of KEEPs launches nothing.
 * Levels: j_max is the level count the forward transform RETURNED (its `*j`).  j_max < 0 stands for what the transforms
 * give these sizes by default (ceil(log2) of the smaller side; of the length of a single row or column) and a j_max
 * beyond ceil(log2) of the larger side is cut to that; dwt_hip_band_levels returns the count a call will use, and the
 * tables hold dwt_hip_band_slots(that count) entries.
 * `ptr` may be host or device memory; `ops` / `params` are HOST arrays.  Dense device frames (stride_y == 4) run where
 * they lie, host frames and other strides are staged through a dense device image and only the frame's own elements are
 * written back.  Calls are ordered on the context's stream.  Bad sizes, a null table or an unknown operator return an
 * error and launch nothing. */
enum dwt_hip_band_op {
	DWT_HIP_BAND_KEEP = 0,
	DWT_HIP_BAND_ZERO,
	DWT_HIP_BAND_SCALE,
	DWT_HIP_BAND_HARD,
	DWT_HIP_BAND_SOFT,
	DWT_HIP_BAND_COMPRESS
};
#define DWT_HIP_BAND_MAX_SLOTS 94 /* 3 * 31 + 1: no table is longer */
/* 3 * j_max + 1 (-1 for j_max outside 0 .. 31) */
int dwt_hip_band_slots(int j_max);
/* the level count the band entries use for a frame of these outer sizes and this j_max (-1: bad sizes) */
int dwt_hip_band_levels(int size_o_x, int size_o_y, int j_max);
/* {x, y, size_x, size_y} of every slot, in elements from the frame's origin -> xywh (4 ints per slot); returns the slot
 * count, -1 for bad sizes */
int dwt_hip_band_geometry(int size_o_x, int size_o_y, int size_i_x, int size_i_y, int j_max, int *xywh);
int dwt_hip_bands_apply(void *ptr, int stride_x, int stride_y, int size_o_x, int size_o_y, int size_i_x, int size_i_y,
	int j_max, const int *ops, const float *params);
/* `batch` dense frames (size_o == size_i) batch_stride bytes apart.  table_stride 0: one table for all frames;
 * otherwise frame b reads ops + b * table_stride and params + b * table_stride (per-image thresholds) -- still ONE
 * launch (the tables cross to the device in one small copy). */
int dwt_hip_bands_apply_batch(void *ptr, size_t batch_stride, int batch, int stride_x, int size_x, int size_y, int j_max,
	const int *ops, const float *params, size_t table_stride);
/* The pointwise maps of the hdr flow over a frame or a batch of frames, in place, one launch:
 *   LOG  (float)log((double)(c + a)), c + a the float sum        (the reference's logf(*c + eps))
 *   EXP  (float)exp((double)c) - a, a float subtraction          (expf(*c) - eps)
 * NaN stays NaN.  Memory spaces as above. */
enum dwt_hip_map_op { DWT_HIP_MAP_LOG = 0, DWT_HIP_MAP_EXP };
int dwt_hip_map(int op, void *ptr, int stride_x, int stride_y, int size_x, int size_y, float a);
int dwt_hip_map_batch(int op, void *ptr, size_t batch_stride, int batch, int stride_x, int size_x, int size_y, float a);
/* The universal threshold of every frame of a batch of transformed dense frames -> lambda (HOST memory, one per frame):
 *   lambda = (med / 0.6745f) * sqrtf(2.f * logf((float)(size_x * size_y))),
 * med the median magnitude of the Mallat HH(1) band (the element of rank n/2 of |c|, as dwt_util_abs_s +
 * dwt_util_band_med_s give it on a copy), finished in float as the reference's denoise_estimate_threshold writes it.  The
 * frames are only read.  NOT a drop-in for that function, which addresses HH(1) as element (1, 1) with both strides
 * 2 * stride_x and so reads past the frame of every real image. */
int dwt_hip_universal_threshold_batch(const void *ptr, size_t batch_stride, int batch, int stride_x, int size_x, int size_y,
	float *lambda);

/* N-term approximation: keep the coefficients of the N largest magnitudes, zero the rest -- the non-linear branch of the
 * reference's examples/displ-vectors/vectors.c (:254-297), on coefficients that stay where they lie.
 * A GROUP is `channels` (1 .. 4) dense float frames of size_x x size_y, the transforms of the channels of one image:
 * channel c of group g at ptr + g*batch_stride + c*channel_stride, rows stride_x bytes apart.  Groups may follow each
 * other (batch_stride spans a group) or every channel's frames may (channel_stride spans the batch).
 *   SCOPE      FRAME: every position of the frame (what vectors.c does; j_max is ignored).  DETAILS: every position
 *              outside the coarsest approximation band, the rectangle x < ceil(size_x / 2^J) && y < ceil(size_y / 2^J)
 *              with J = dwt_hip_band_levels(size_x, size_y, j_max).  M positions are in scope.
 *   MAGNITUDE  of a position, in float, every product and sum rounded on its own (no FMA), summed left to right, the
 *              root correctly rounded: fabsf(c0) for one channel; sqrtf(c0*c0 + c1*c1) for two (vectors.c:261-264);
 *              sqrtf((c0*c0 + c1*c1) + c2*c2) for three; one more term, added the same way, for four.
 *   THRESHOLD  n = keep[g], and n = M where n < 1 or n > M (:281-283); thr is element n-1 of the scope's magnitudes
 *              sorted in descending order (:279, :285).
 *   APPLY      every position in scope with magnitude < thr gets +0.0f in every channel (:292-296); every other
 *              coefficient keeps its bits.  Ties at thr are all kept: kept[g], the positions in scope with magnitude
 *              >= thr, can exceed n.  Positions outside the scope and the bytes between a row's end and its pitch are
 *              neither read for the decision nor written.
 * M == 0 (DETAILS with J == 0, an empty frame) gives thr = 0, kept = 0, launches nothing and writes nothing.  A group
 * that holds a NaN is not pinned (the reference's comparator is no order there); the call returns normally and the
 * other groups of the batch are exact.  Infinities, overflowing squares and subnormals follow from the arithmetic.
 * `ptr` may be host or device memory; `keep`, `thr` and `kept` are HOST arrays of `batch` entries, thr and kept may be
 * NULL.  Dense device frames run where they lie, in at most 5 kernel launches whatever batch, channels and n; host
 * frames and other element strides are staged through a dense device image and only the frames' own elements are
 * written back.  Calls are ordered on the context's stream; with thr == NULL && kept == NULL a call on device frames
 * does not wait for the device.  A null pointer, channels outside 1 .. 4, an unknown scope, negative sizes, more than
 * INT_MAX positions in a frame, a pitch below its row, frames or channels closer than they span, thr or kept in device
 * memory or a device address or stride that is no multiple of 4 return an error, launch nothing and write nothing. */
enum dwt_hip_nterm_scope { DWT_HIP_NTERM_FRAME = 0, DWT_HIP_NTERM_DETAILS = 1 };
int dwt_hip_keep_largest_batch(void *ptr, size_t batch_stride, int batch, int channels, size_t channel_stride, int stride_x,
	int size_x, int size_y, int j_max, int scope, const int *keep, float *thr, int *kept);
/* one frame of one channel, element (y, x) at ptr + y*stride_x + x*stride_y (host or device): the calling convention of
 * dwt_hip_bands_apply */
int dwt_hip_keep_largest(void *ptr, int stride_x, int stride_y, int size_x, int size_y, int j_max, int scope, int keep, float *thr,
	int *kept);
/* The magnitude map alone (vectors.c's `map`), one launch; the frames are only read.  The map of group g goes to
 * map + g*map_batch_stride, rows map_stride_x bytes apart, dense elements.  Frames and map lie both in host or both in
 * device memory and must not overlap. */
int dwt_hip_magnitude_batch(const void *ptr, size_t batch_stride, int batch, int channels, size_t channel_stride, int stride_x,
	int size_x, int size_y, void *map, size_t map_batch_stride, int map_stride_x);

/* The stationary (undecimated) wavelet transform of rows: swt_cdf97_f_ex_stride_s / swt_cdf53_f_ex_stride_s (src/swt.c),
 * every level of a batch of lines in one call.  Level l (0-based) filters the low-pass plane of level
 * l-1 (level 0: the input) with the low-pass and the high-pass filter dilated by 1 << l, borders replicated; every plane
 * has N samples.  `wavelet` is DWT_HIP_CDF97_S or DWT_HIP_CDF53_S.  `levels` runs from 0 (nothing is written) to
 * DWT_HIP_SWT_MAX_LEVELS; dilations beyond N are legal.  Lines are line_stride bytes apart, their elements elem_stride.
 * H of level l of line y goes to dst_h + l*plane_stride + y*dst_line_stride (bytes), dense in x.  l_mode 0: no L is
 * written (dst_l may be NULL); 1: only the last level's L, to plane 0 of dst_l; 2: every level's L, laid out like H.
 * All pointers are host memory or all device memory.  src is never written; src, dst_h and dst_l must not overlap (an
 * error).  Device lines of dense elements and up to 8192 samples take ONE kernel launch whatever `levels` and n_lines;
 * longer lines and strided elements one launch per level.  Output is bit-identical to the reference's over the whole
 * float range. */
#define DWT_HIP_SWT_MAX_LEVELS 24
int dwt_hip_swt1d_batch(int wavelet, const void *src, size_t line_stride, size_t elem_stride, int n_lines, int N, int levels,
	void *dst_h, void *dst_l, int l_mode, size_t plane_stride, size_t dst_line_stride);
/* ONE level at dilation 1 << level of one line, as the reference's entry takes it (include/swt.h): src, dst_l and dst_h
 * have N elements `stride` bytes apart; level 0 .. DWT_HIP_SWT_MAX_LEVELS-1 */
int dwt_hip_swt1d_level(int wavelet, const void *src, void *dst_l, void *dst_h, int N, int stride, int level);
/* The stationary wavelet transform of image batches: the two functions above applied separably.  Level l
 * (0-based, dilation 1 << l) filters its input A -- the image at level 0, LL of level l-1 after that -- along x for every
 * row, Lr = conv_x(A, low), Hr = conv_x(A, high), and then along y for every column: LL = conv_y(Lr, low), LH =
 * conv_y(Lr, high), HL = conv_y(Hr, low), HH = conv_y(Hr, high); borders replicated, no direction ever skipped (a 1-row
 * image takes its column pass with N = 1), every plane size_x x size_y.  Band names as enum dwt_subbands: HL is high-pass
 * along a row.  The inverse is dwt_hip_iswt2d_batch, under the symmetric border of dwt_hip_swt2d_batch_ex (replicated
 * borders do not reconstruct).  stride_x is the row pitch and stride_y the element pitch of src in bytes; images are
 * batch_stride bytes apart.  Detail band k (HL = 1, LH = 2, HH = 3) of level l of image b goes to
 *     dst_h + b*dst_batch_stride + (3*l + k-1)*plane_stride + y*dst_stride_x + 4*x.
 * l_mode 0: no LL is written (dst_l may be NULL); 1: the last level's LL, to plane 0 of dst_l + b*dst_batch_stride;
 * 2: level l's LL to plane l there.  `levels` runs from 0 (nothing is written) to DWT_HIP_SWT_MAX_LEVELS; dilations beyond
 * either size are legal.  dst_h and dst_l share dst_batch_stride: dst_l needs batch * dst_batch_stride bytes of its own, or
 * lies in the gap behind every image's detail planes.  All pointers are host memory or all device memory.  src is never written; src, dst_h and dst_l
 * must not overlap, planes and images must be apart, a pitch must hold its row, batch and both sizes are at least 1
 * (errors otherwise).  Dense device images (stride_y 4) take ONE kernel launch per level for the whole batch on levels
 * 0 .. DWT_HIP_SWT2D_FUSED_LEVELS-1; strided elements, deeper levels and every call under option "swt2d_fused" = 0 take
 * two (a row pass and a column pass through library scratch).  Output is bit-identical to the reference's functions run
 * over the rows and then over the columns, over the whole float range. */
#define DWT_HIP_SWT2D_FUSED_LEVELS 5
#define DWT_HIP_SWT2D_TILE_W 256 /* the fused kernel's tile: columns, and rows of the level's row lattice y0 + (i << l) */
#define DWT_HIP_SWT2D_TILE_H 32
int dwt_hip_swt2d_batch(int wavelet, const void *src, size_t batch_stride, int batch, int stride_x, int stride_y, int size_x, int size_y,
	int levels, void *dst_h, void *dst_l, int l_mode, size_t dst_batch_stride, size_t plane_stride, int dst_stride_x);
/* ONE level at dilation 1 << level of one image: the four planes have rows dst_stride_x and elements dst_stride_y bytes
 * apart; level 0 .. DWT_HIP_SWT_MAX_LEVELS-1.  src and the four planes must not overlap. */
int dwt_hip_swt2d_level(int wavelet, const void *src, int stride_x, int stride_y, int size_x, int size_y, int level, void *dst_ll,
	void *dst_hl, void *dst_lh, void *dst_hh, int dst_stride_x, int dst_stride_y);
/* The border rule of the stationary transforms.  REPLICATE is the reference's: x[clamp(i)].  SYMMETRIC is whole-sample
 * symmetric extension, x[reflect(i)] with reflect(i, N) = 0 for N = 1 and otherwise m = i mod 2(N-1) taken non-negative,
 * m > N-1 ? 2(N-1) - m : m: an extension, and the rule under which the transform has an inverse -- the
 * filters are symmetric and of odd length, so every plane of a symmetrically extended input is itself symmetric about
 * samples 0 and N-1 at every dilation.  Away from the borders (CL * (2^J - 1) samples after J levels) both rules give the
 * same coefficients. */
enum dwt_hip_swt_border {
	DWT_HIP_SWT_BORDER_REPLICATE = 0,
	DWT_HIP_SWT_BORDER_SYMMETRIC = 1
};
/* dwt_hip_swt1d_batch / dwt_hip_swt2d_batch with the border rule as their last argument; border 0 is those entries. */
int dwt_hip_swt1d_batch_ex(int wavelet, const void *src, size_t line_stride, size_t elem_stride, int n_lines, int N, int levels,
	void *dst_h, void *dst_l, int l_mode, size_t plane_stride, size_t dst_line_stride, int border);
int dwt_hip_swt2d_batch_ex(int wavelet, const void *src, size_t batch_stride, int batch, int stride_x, int stride_y, int size_x, int size_y,
	int levels, void *dst_h, void *dst_l, int l_mode, size_t dst_batch_stride, size_t plane_stride, int dst_stride_x, int border);
/* The inverse stationary transform of rows (an extension: the reference has none).  `border` must be
 * DWT_HIP_SWT_BORDER_SYMMETRIC: replicated borders do not reconstruct (an error).  src_h is laid out as dwt_hip_swt1d_batch
 * writes dst_h -- H of level l of line y at src_h + l*plane_stride + y*src_line_stride, dense -- and src_l holds the last
 * level's L lines src_line_stride bytes apart (a caller with an l_mode 2 buffer passes the address of its last plane).
 * Levels run from levels-1 down to 0, level l at dilation u = 1 << l:
 *     x = 0.5f * (conv(L, sl, u) + conv(H, sh, u)),   sl[i] = (-1)^(i-CH) * gh[i],   sh[i] = (-1)^(i-CL) * gl[i],
 * every conv the forward's tap sum over reflected indices (float32, each product and sum rounded on its own).  The result
 * goes to dst, lines dst_line_stride and elements dst_elem_stride bytes apart.  `ops` and `params` are optional host tables
 * of `levels` entries, one operator (DWT_HIP_BAND_KEEP, _ZERO, _SCALE, _HARD, _SOFT; _COMPRESS is an error) and one
 * parameter per H plane, both NULL for KEEP everywhere: a detail coefficient passes through its operator as it is read, and
 * the result is bit for bit that of applying the operator to the stored plane first.  A ZERO plane is never read.
 * levels = 0 copies src_l to dst.  All pointers are host memory or all device memory; dst must not overlap src_h or src_l;
 * levels 0 .. DWT_HIP_SWT_MAX_LEVELS; a refused call writes nothing.  Dense device lines of up to 8192 samples take ONE
 * kernel launch whatever `levels` and n_lines; longer lines, strided dst elements and option "swt_fused" = 0 one per level.
 * A forward transform under the symmetric border followed by this call returns the input within 1e-6 * max|x| for normal
 * inputs (the filters' 8-digit literals and float32 rounding; it is no bit-exact pair). */
int dwt_hip_iswt1d_batch(int wavelet, int border, const void *src_h, const void *src_l, size_t plane_stride, size_t src_line_stride,
	int n_lines, int N, int levels, const int *ops, const float *params, void *dst, size_t dst_line_stride, size_t dst_elem_stride);
/* The inverse stationary transform of image batches: columns first, then rows (the forward order reversed),
 *     Lr = 0.5f*(conv_y(LL, sl) + conv_y(LH, sh))   Hr = 0.5f*(conv_y(HL, sl) + conv_y(HH, sh))   A = 0.5f*(conv_x(Lr, sl) + conv_x(Hr, sh)).
 * The detail planes are laid out as dwt_hip_swt2d_batch writes them -- band k of level l of image b at
 * src_h + b*src_batch_stride + (3*l + k-1)*plane_stride + y*src_stride_x + 4*x -- and src_l is the last level's LL of
 * every image, at src_l + b*src_batch_stride + y*src_stride_x + 4*x.  The result goes to dst + b*dst_batch_stride +
 * y*dst_stride_x + x*dst_stride_y.  `ops` / `params`: as above with 3 * levels entries, the plane's at index 3*l + k-1.  The
 * intermediate LL planes live in library scratch.  Dense device destinations take ONE kernel launch per level for the whole
 * batch on levels 0 .. DWT_HIP_ISWT2D_FUSED_LEVELS-1; deeper levels, strided dst elements and option "swt2d_fused" = 0 take
 * two (a column pass and a row pass through library scratch).  Otherwise the rules of the row entry.  Round trip of normal
 * inputs: within 2e-6 * max|x|. */
#define DWT_HIP_ISWT2D_FUSED_LEVELS 5
int dwt_hip_iswt2d_batch(int wavelet, int border, const void *src_h, const void *src_l, size_t src_batch_stride, size_t plane_stride,
	int src_stride_x, int batch, int size_x, int size_y, int levels, const int *ops, const float *params, void *dst,
	size_t dst_batch_stride, int dst_stride_x, int dst_stride_y);
/* The feature statistics of the transform's planes without the planes: feature k of the mask (enum order) of level l of
 * line y at fv[y*fv_line_stride + k*levels + l] (floats).  band 0: the H planes, 1: the L planes.  Each value is what
 * dwt_util_band_<name>_s(plane, 0, sizeof(float), N, 1[, p]) gives for that plane, wps with j = l.  fv lies where src
 * lies (host or device).  Lines the one-launch kernel takes are reduced in that launch and no coefficient is stored.  Like
 * the other feature entries the call waits for its stream: the sums are finished on the host. */
int dwt_hip_swt_features1d_batch(int wavelet, unsigned feature_mask, const void *src, size_t line_stride, size_t elem_stride,
	int n_lines, int N, int levels, int band, float p, float *fv, int fv_line_stride);

/* Wavelet packet transforms of row and image batches: every node is split again at every level, not only
 * the L node.  An extension: the reference has no packet driver; a packet level is its own one-level transform applied to
 * each node.  `wavelet` is DWT_HIP_CDF97_S, DWT_HIP_CDF53_S or DWT_HIP_INTERP53_S (anything else is an error).
 *
 * Node tree of a line of N samples, natural (Paley) order: level 0 has the node [0, N); the node [s, s+n) of level j has
 * its L child at [s, s+ceil(n/2)) and its H child at [s+ceil(n/2), s+n) of level j+1.  The natural index k reads the path,
 * first split in the most significant bit (0 = L).  Node k of level j has (N - bitrev_j(k) + 2^j - 1) >> j samples, the
 * starts are the prefix sums.  Forward level j: one call of the reference's one-level line function
 * (dwt_cdf97_f_ex_stride_s and its siblings) per node of level j, dst_l at s and dst_h at s + ceil(n/2); after `levels`
 * levels the line holds its 2^levels leaves in natural order.  The inverse is the mirror, levels-1 .. 0, each node rebuilt
 * by the one-level inverse line function.  1 <= levels <= floor(log2 N): every node that is split has two samples or more
 * (anything else is an error, not clamped).  In 2-D the node rectangles are the product of the rule along x and along y,
 * node (ky, kx); a forward level gives every node one level of dwt_cdf97_2f_s (dwt_cdf53_2f_s, dwt_interp53_2f_s) on an
 * image of the node's size -- rows, then columns, LL | HL over LH | HH inside the node's rectangle --, the inverse one level
 * of the matching _2i_s (rows, then columns);  1 <= levels <= min(floor(log2(min(size_x, size_y))), 8).
 * The band of natural node k is not the k-th lowest: dwt_hip_wp_freq_order gives the Gray code perm[f] = f ^ (f >> 1), the
 * natural index of the node with the f-th lowest band (per axis in 2-D).  Data is never permuted.
 *
 * src == dst is in place; otherwise dst receives the transform and src is left untouched (they must not overlap).  Both
 * are host memory (synchronous) or both device memory (ordered on the context's stream, no synchronisation, no allocation
 * after the first call of a shape).  Lines are line_stride bytes apart, their elements elem_stride; images batch_stride
 * apart, rows stride_x, elements stride_y; only the frame's own elements are written.  Lines lie apart (line_stride >=
 * (N-1)*elem_stride + 4) or interleaved inside one element step (n_lines*line_stride <= elem_stride: line y the channel y
 * of an array of n_lines or more channels); anything else, where two lines would share a sample, is an error.  Device lines of up to 8192 samples
 * take ONE kernel launch whatever `levels` and n_lines; dense device images (stride_y 4) one launch per level for the whole
 * batch.  Longer lines, strided image elements and every call under option "wp_fused" = 0 run level by level through the
 * exact line passes, node by node.  Same bits on every route: those of the reference's functions per node, over the whole
 * float range. */
/* natural-order node table of one level of an N-sample line: start[k], len[k] for k < 2^level (either may be NULL);
 * returns 2^level, -1 for bad arguments (level > floor(log2 N)) */
int dwt_hip_wp_nodes(int N, int level, int *start, int *len);
/* perm[f] = natural index of the f-th lowest band (perm may be NULL); returns 2^level, -1 for a level outside 0 .. 30 */
int dwt_hip_wp_freq_order(int level, int *perm);
int dwt_hip_wp1d_batch(int wavelet, int inverse, const void *src, void *dst, size_t line_stride, size_t elem_stride,
	int n_lines, int N, int levels);
int dwt_hip_wp2d_batch(int wavelet, int inverse, const void *src, void *dst, size_t batch_stride, int batch,
	int stride_x, int stride_y, int size_x, int size_y, int levels);
/* statistics of every node of `level` of transformed packet lines / images, node order natural (order = 0) or
 * frequency (1; 2-D: node (perm[fy], perm[fx]) at fy * 2^level + fx); the contracts of dwt_hip_features1d_batch /
 * _2d_batch (fv in the memory space of ptr, fixed-order double sums, the Band's j = level): per line / image one block of
 * 2^level (4^level) floats per feature of the mask in enum order.  At most 96 nodes: level <= 6 in 1-D, <= 3 in 2-D (more
 * is an error). */
int dwt_hip_wp_features1d_batch(unsigned feature_mask, const void *ptr, size_t line_stride, size_t elem_stride,
	int n_lines, int N, int level, int order, float p, float *fv, size_t fv_stride);
int dwt_hip_wp_features2d_batch(unsigned feature_mask, const void *ptr, size_t batch_stride, int batch, int stride_x,
	int size_x, int size_y, int level, int order, float p, float *fv, size_t fv_stride);

/* Best basis and pruned wavelet packet trees of row batches (images: further down).  An extension, like the packets
 * themselves: a leaf of a pruned tree holds, bit for bit, what that node holds in the full tree of its depth.
 *
 * Trees.  A tree of depth `levels` (1 <= levels <= min(floor(log2 N), DWT_HIP_WP_TREE_MAX_LEVELS)) is a bitmap of
 * DWT_HIP_WP_TREE_WORDS uint32_t (128 bytes whatever `levels`).  Node k (natural index) of level j has the heap index
 * h = 2^j + k; bit h (word h >> 5, bit h & 31) set means "this node is split into (j+1, 2k) and (j+1, 2k+1)".  Bit 0 and the
 * bits of levels >= `levels` mean nothing.  The EFFECTIVE tree is what can be reached from the root through set bits: a set
 * bit below a clear one is ignored, on the host and on the device alike, so a tree in device memory needs no validation and
 * no synchronisation.  Node geometry is that of dwt_hip_wp_nodes; the leaves of any effective tree tile [0, N), and a
 * transformed line holds each leaf (j, k) at [start_j(k), start_j(k) + len_j(k)).
 *
 * Costs.  Additive, one term per coefficient c, evaluated in double with x = (double)c, e = x*x:
 *   DWT_HIP_WP_COST_SHANNON     e == 0 ? 0 : -e*log(e)
 *   DWT_HIP_WP_COST_LOG_ENERGY  e == 0 ? 0 : log(e)
 *   DWT_HIP_WP_COST_LP          |x|^param, 0 < param < 2 (param == 1: fabs(x), no pow)
 *   DWT_HIP_WP_COST_THRESHOLD   |c| > param ? 1 : 0, param >= 0, compared in float
 * The term of a non-finite c is NaN; a bad kind or param is an error.  A node's cost is the sum of its terms in double, in
 * an order that is fixed: the same bits on every run, for every batch size and every position of the line in the batch (no
 * float atomics).  The one-launch route and the cross-check route may differ from each other in rounding.
 *
 * Selection, bottom-up: best[h] = cost[h] at level `levels`; above, c = best[2h] + best[2h+1] (L child first), the node is
 * split iff c < cost[h], then best[h] = c, else best[h] = cost[h].  A tie keeps the parent; so does a NaN on either side
 * (the comparison is false).  Trees that the library writes hold effective bits only.  The total is best[1]. */
#define DWT_HIP_WP_TREE_MAX_LEVELS 10
#define DWT_HIP_WP_TREE_WORDS 32
enum dwt_hip_wp_cost {
	DWT_HIP_WP_COST_SHANNON = 0,
	DWT_HIP_WP_COST_LOG_ENERGY = 1,
	DWT_HIP_WP_COST_LP = 2,
	DWT_HIP_WP_COST_THRESHOLD = 3
};
/* Host helpers, no device.  The best tree of a table of 2^(levels+1) node costs in heap order ([0] unused): the tree
 * (DWT_HIP_WP_TREE_WORDS words) and the total; either output may be NULL.  Returns 0, -1 for bad arguments. */
int dwt_hip_wp_best_tree(int levels, const double *cost, uint32_t *tree, double *total);
/* the leaves of the effective tree from left to right: level, natural index, start and length of each (any array may be
 * NULL; at most 2^levels entries).  Returns the number of leaves, -1 for bad arguments. */
int dwt_hip_wp_tree_leaves(int N, int levels, const uint32_t *tree, int *level, int *index, int *start, int *len);
/* The search: the cost of every node of levels 0 .. `levels` of every line, the best tree of each line and, where dst is
 * not NULL, the line in that tree.  Wavelets, stride rules, the apart-or-interleaved rule, in place (src == dst) and the
 * overlap check are those of dwt_hip_wp1d_batch.  Outputs, each optional, at least one of the four not NULL, all in the
 * memory space of src: dst; tree -- line i's at (char *)tree + i*tree_stride, tree_stride >= 128 bytes and a multiple of 4;
 * total -- n_lines doubles; node_cost -- line i's 2^(levels+1) doubles in heap order, [0] = the total, at (char *)node_cost
 * + i*cost_stride, cost_stride >= 8 * 2^(levels+1) bytes and a multiple of 8.  dst == NULL: costs and tree only, no
 * coefficient is stored.  Device memory: everything is ordered on the context's stream; the entry neither waits for the
 * stream nor reads anything back (the selection runs on the device).  Dense or strided device lines of up to 8192 samples
 * take ONE launch; longer lines and every call under option "wp_fused" = 0 run level by level through the exact line passes
 * and small helper kernels.  Host memory: synchronous, through the staging path. */
int dwt_hip_wp_best1d_batch(int wavelet, int cost, float param, const void *src, void *dst, size_t line_stride, size_t elem_stride,
	int n_lines, int N, int levels, uint32_t *tree, size_t tree_stride, double *total, double *node_cost, size_t cost_stride);
/* The transform in a given tree, forward or inverse (the inverse rebuilds exactly the nodes that the tree splits).  tree in
 * the memory space of src, line i's at (char *)tree + i*tree_stride; tree_stride 0: one tree for every line.  Everything
 * else as dwt_hip_wp1d_batch; with the full tree of depth `levels` the bits are those of dwt_hip_wp1d_batch. */
int dwt_hip_wp_tree1d_batch(int wavelet, int inverse, const void *src, void *dst, size_t line_stride, size_t elem_stride, int n_lines,
	int N, int levels, const uint32_t *tree, size_t tree_stride);

/* Best basis and pruned packet QUADTREES of image batches: the 2-D twin of the four entries above.
 *
 * Quadtrees.  Node (ky, kx) of level j has the rectangle that dwt_hip_wp_nodes gives along y (index ky, of size_y) and along
 * x (index kx, of size_x): the geometry of dwt_hip_wp2d_batch.  Its quadtree index is q = (4^j - 1)/3 + ky*2^j + kx; the
 * root is 0.  Its children, in this order: LL (j+1, 2ky, 2kx), HL (j+1, 2ky, 2kx+1), LH (j+1, 2ky+1, 2kx), HH (j+1, 2ky+1,
 * 2kx+1).  A tree of depth `levels` is a bitmap of DWT_HIP_WP_QTREE_WORDS uint32_t (64 bytes whatever `levels`): bit q
 * (word q >> 5, bit q & 31) set means "this node is split into its four children".  The bits of levels >= `levels` mean
 * nothing.  The EFFECTIVE tree is what can be reached from the root through set bits: a set bit below a clear one is
 * ignored, on the host and in every kernel, so a tree in device memory needs no validation and no synchronisation, and
 * the library writes effective bits only.  1 <= levels <= min(floor(log2(min(size_x, size_y))),
 * DWT_HIP_WP_QTREE_MAX_LEVELS); anything else is an error, not a clamp.  The leaves of any effective tree tile the image,
 * and a leaf (j, ky, kx) holds, bit for bit, what that node holds after dwt_hip_wp2d_batch with levels = j, at the
 * node's place.
 *
 * Costs are the four kinds of enum dwt_hip_wp_cost with the terms and parameter checks stated above: double, NaN for a
 * non-finite coefficient.  A node's cost is the double sum of its terms in a fixed order that is a function of size_x,
 * size_y, the level and the node alone -- not of the batch size, the image's position in the batch or the run (no float
 * or double atomics).  The fused route and the cross-check route may differ from each other in rounding.
 *
 * Selection, bottom-up: best[q] = cost[q] at level `levels`; above, c = ((best[LL] + best[HL]) + best[LH]) + best[HH],
 * the node is split iff c < cost[q], then best[q] = c, else best[q] = cost[q].  A tie keeps the parent; so does a NaN on
 * either side.  The total is best[0]. */
#define DWT_HIP_WP_QTREE_MAX_LEVELS 5
#define DWT_HIP_WP_QTREE_WORDS 16
/* Host helpers, no device.  The best quadtree of a table of (4^(levels+1) - 1)/3 node costs in index order: the tree
 * (DWT_HIP_WP_QTREE_WORDS words) and the total; either output may be NULL.  Returns 0, -1 for bad arguments. */
int dwt_hip_wp_best_qtree(int levels, const double *cost, uint32_t *tree, double *total);
/* the leaves of the effective tree, depth first with the children in the order LL, HL, LH, HH: level, ky, kx and the
 * rectangle (x0, y0, w, h) of each (any array may be NULL; at most 4^levels entries).  Returns the number of leaves, -1
 * for bad arguments. */
int dwt_hip_wp_qtree_leaves(int size_x, int size_y, int levels, const uint32_t *tree, int *level, int *ky, int *kx, int *x0, int *y0,
	int *w, int *h);
/* The search: the cost of every node of levels 0 .. `levels` of every image, the best quadtree of each image and, where
 * dst is not NULL, the image in that tree.  Wavelets, stride rules, in place (src == dst), the overlap check, the batch
 * cap and the memory-space rule are those of dwt_hip_wp2d_batch.  Outputs, each optional, at least one of the four not
 * NULL, all in the memory space of src: dst; tree -- image i's at (char *)tree + i*tree_stride, tree_stride >= 64 bytes
 * and a multiple of 4; total -- `batch` doubles; node_cost -- image i's (4^(levels+1) - 1)/3 doubles in index order at
 * (char *)node_cost + i*cost_stride, cost_stride at least that many doubles and a multiple of 8 bytes.  dst == NULL: costs
 * and tree only, no coefficient is stored.  Device memory: everything is ordered on the context's stream; the entry
 * neither waits for the stream nor reads anything back (the selection runs on the device).  Dense device images (stride_y
 * 4, every address and stride a multiple of 4 bytes) take 2*levels + 2 launches, 3*levels + 2 with dst, whatever the
 * batch and the shape; strided elements, host memory and every call under option "wp_fused" = 0 run the staged frame
 * level by level through the exact line passes and small helper kernels.  Host memory: synchronous. */
int dwt_hip_wp_best2d_batch(int wavelet, int cost, float param, const void *src, void *dst, size_t batch_stride, int batch,
	int stride_x, int stride_y, int size_x, int size_y, int levels, uint32_t *tree, size_t tree_stride, double *total,
	double *node_cost, size_t cost_stride);
/* The transform in given quadtrees, forward or inverse (the inverse rebuilds exactly the nodes that the effective tree
 * splits).  tree in the memory space of src, image i's at (char *)tree + i*tree_stride; tree_stride 0: one tree for every
 * image.  Everything else as dwt_hip_wp2d_batch; with the full tree of depth `levels` the bits are those of
 * dwt_hip_wp2d_batch.  Dense device images take one launch per level. */
int dwt_hip_wp_tree2d_batch(int wavelet, int inverse, const void *src, void *dst, size_t batch_stride, int batch, int stride_x,
	int stride_y, int size_x, int size_y, int levels, const uint32_t *tree, size_t tree_stride);

/* The pixel front end: pictures of 8- or 16-bit unsigned pixels <-> the planes the 2-D transforms take,
 * with the DC level shift and the component transforms of ITU-T T.800 Annex G.  An extension: the reference's picture
 * programs widen the pixels on the host and hand over one channel at a time.
 *
 * Pixels.  `fmt` DWT_HIP_PIX_U8 or _U16 (host byte order), `channels` 1, 3 or 4.  Channel c of pixel (x, y) of picture b
 * lies at pix + b*pix_batch_stride + y*pix_row_pitch + x*pix_stride + c*chan_stride, all in bytes: interleaved RGB8 is
 * pix_stride 3, chan_stride 1; BGRA8 is 4, 1 with order DWT_HIP_ORDER_BGR; planar is pix_stride = element size,
 * chan_stride = plane bytes; three used channels of a 4-byte pixel is 4, 1, channels 3.  Any byte alignment is legal; no
 * two elements may share a byte (the three steps must nest in some order).  `order` says which of the first three channels
 * is R.  A fourth channel takes offset and scale only, never the component transform.
 *
 * Planes.  Plane (b, c) lies at planes + (b*channels + c)*plane_stride, rows plane_row_pitch bytes apart, elements
 * adjacent; `plane_type` DWT_HIP_PLANE_I16, _I32, _H (binary16) or _S (binary32); addresses and strides are multiples of
 * the element size.  After a component transform component 0 is Y, 1 is Cb / U, 2 is Cr / V whatever `order` was.
 *
 * Forward.  depth is 1 .. 8 (u8) or 1 .. 16 (u16); pixel values are used as stored.  v = pix - offset (offset an int,
 * usually 2^(depth-1)).  Integer planes (scale must be 1): DWT_HIP_COLOUR_NONE stores v; _RCT stores Y = (R + 2G + B) >> 2,
 * U = B - G, V = R - G in 32-bit wrapping arithmetic with an arithmetic shift, truncated to the plane's width.  Float
 * planes: v converted to binary32 (to nearest even), times scale; _ICT then stores
 *     Y  = (0.299f*R + 0.587f*G) + 0.114f*B
 *     Cb = (-0.16875f*R + -0.33126f*G) + 0.5f*B
 *     Cr = (0.5f*R + -0.41869f*G) + -0.08131f*B
 * every product and sum rounded to binary32 on its own, in this order; _H planes round the result to binary16 once, to
 * nearest even.
 *
 * Inverse.  Integer planes widen to int; _RCT: G = Y - ((U + V) >> 2), R = V + G, B = U + G, wrapping; + offset
 * (wrapping), clamped to [0, 2^depth - 1].  Float planes widen exactly; _ICT: R = Y + 1.402f*Cr,
 * G = (Y + -0.34413f*Cb) + -0.71414f*Cr, B = Y + 1.772f*Cb; times the call's scale (the caller passes the reciprocal of
 * the forward one); rounded to the nearest integer, ties to even; + offset (exactly); clamped.  NaN gives 0, +-Inf the
 * ends of the range.
 *
 * Errors (nonzero, dwt_hip_last_error, nothing written): RCT with float planes, ICT or scale != 1 with integer planes, a
 * component transform with fewer than 3 channels, RCT into _I16 at depth 16 (U and V need depth + 1 bits), a depth
 * outside the pixel type, 2 or 5+ channels, pixels and planes that overlap, elements that share bytes.
 *
 * Each side is host or device memory on its own.  Device sides are ordered on the context's stream: one kernel launch, no
 * synchronisation, no allocation.  A host side is mirrored in a device buffer of the context (its whole region crosses
 * PCIe; a written region with bytes outside the frame is uploaded first so that they come back as they were) and the call
 * ends synchronised.  Only the frame's own elements change.  A lane converts DWT_HIP_PIXELS_PER_LANE consecutive pixels of
 * a row; a side whose base, pitches and strides are multiples of 16 bytes moves by 16-byte accesses, any other side
 * element by element (option "pixels_wide" = 0: every side): same bits.  dwt_hip_pixels_route tells which: the OR of
 * DWT_HIP_PIXELS_WIDE_PIX and _WIDE_PLANES for a call with these addresses, -1 for arguments the entries refuse.  The answer
 * holds for the device sides of the two conversion entries: a host side runs on its mirror, whose base is aligned whatever
 * the host address was, and the composite entries convert into or out of their scratch stack, not the caller's planes.
 * A wide load of an interleaved pixel that has more elements than channels (three channels of a 4-element pixel, grey
 * at a 3- or 4-element step) reads the pixel's unused elements too, the last pixel's up to 3 (u8) or 6 (u16) bytes past the
 * frame's last element -- inside the same aligned 16 bytes, never written. */
enum dwt_hip_pixel_format { DWT_HIP_PIX_U8 = 0, DWT_HIP_PIX_U16 = 1 };
enum dwt_hip_pixel_order { DWT_HIP_ORDER_RGB = 0, DWT_HIP_ORDER_BGR = 1 };
enum dwt_hip_colour { DWT_HIP_COLOUR_NONE = 0, DWT_HIP_COLOUR_RCT = 1, DWT_HIP_COLOUR_ICT = 2 };
enum dwt_hip_plane_type { DWT_HIP_PLANE_I16 = 0, DWT_HIP_PLANE_I32 = 1, DWT_HIP_PLANE_H = 2, DWT_HIP_PLANE_S = 3 };
#define DWT_HIP_PIXELS_PER_LANE 16
#define DWT_HIP_PIXELS_GRID_ROWS 16384 /* rows / pictures one trip of the kernel's loops covers */
#define DWT_HIP_PIXELS_GRID_BATCH 4096
#define DWT_HIP_PIXELS_WIDE_PIX 1
#define DWT_HIP_PIXELS_WIDE_PLANES 2
int dwt_hip_pixels_to_planes_batch(int fmt, const void *pix, size_t pix_batch_stride, size_t pix_row_pitch, size_t pix_stride,
	size_t chan_stride, int batch, int channels, int order, int depth, int offset, float scale, int colour, int plane_type,
	void *planes, size_t plane_stride, size_t plane_row_pitch, int size_x, int size_y);
int dwt_hip_planes_to_pixels_batch(int fmt, void *pix, size_t pix_batch_stride, size_t pix_row_pitch, size_t pix_stride,
	size_t chan_stride, int batch, int channels, int order, int depth, int offset, float scale, int colour, int plane_type,
	const void *planes, size_t plane_stride, size_t plane_row_pitch, int size_x, int size_y);
int dwt_hip_pixels_route(int fmt, int inverse, const void *pix, size_t pix_batch_stride, size_t pix_row_pitch, size_t pix_stride,
	size_t chan_stride, int batch, int channels, int plane_type, const void *planes, size_t plane_stride,
	size_t plane_row_pitch, int size_x, int size_y);
/* The conversion and dwt_hip_transform2d_batch of the batch*channels planes (batch_stride = plane_stride, stride_x =
 * plane_row_pitch) in one call: forward the pixels to transformed planes, *j as that entry takes it (levels wanted, -1
 * all; levels done stored); inverse the planes, which are only read, to pixels.  The plane type follows from `wavelet`:
 * DWT_HIP_CDF53_I16 -> _I16; _CDF53_I, _CDF97_I -> _I32; _CDF97_H -> _H; _CDF97_S, _CDF53_S, _INTERP53_S -> _S; the double
 * wavelets are refused, and so are more than 65535 planes, a plane_stride below size_y rows and a plane_row_pitch of 2 GiB
 * or more.  A call that runs no level (*j == 0, or a picture one pixel wide or high) is the conversion alone, *j = 0 stored.
 * Otherwise the samples pass through
 * a scratch stack of planes of the context with the caller's strides (the batched transform runs out of place).  Same bits
 * as the two calls. */
int dwt_hip_picture_forward_batch(int wavelet, int fmt, const void *pix, size_t pix_batch_stride, size_t pix_row_pitch,
	size_t pix_stride, size_t chan_stride, int batch, int channels, int order, int depth, int offset, float scale, int colour,
	void *planes, size_t plane_stride, size_t plane_row_pitch, int size_x, int size_y, int *j);
int dwt_hip_picture_inverse_batch(int wavelet, int fmt, void *pix, size_t pix_batch_stride, size_t pix_row_pitch,
	size_t pix_stride, size_t chan_stride, int batch, int channels, int order, int depth, int offset, float scale, int colour,
	const void *planes, size_t plane_stride, size_t plane_row_pitch, int size_x, int size_y, int j);

/* Deadzone quantization of coefficient planes: the float coefficients of the irreversible path (ICT +
 * DWT_HIP_CDF97_S / _H) <-> sign-magnitude integer indices, the deadzone scalar quantizer of ITU-T T.800 Annex E with one
 * step per subband, plus the two summaries a coder asks for next.  An extension: the reference has no quantizer; this
 * comment is the specification (tests/quant_model.py restates it in numpy, the device is held to it bit for bit).
 *
 * Frames.  `batch` dense Mallat frames of size_x x size_y samples (size_o == size_i, elements adjacent): sample (x, y) of
 * frame b lies at coef + b*coef_batch_stride + y*coef_row_pitch + x*(2 or 4) and at index + b*index_batch_stride +
 * y*index_row_pitch + x*(2 or 4), all in bytes.  `coef_type` DWT_HIP_COEF_S (binary32) or _H (binary16), `index_type`
 * DWT_HIP_INDEX_I16 or _I32; addresses and strides are multiples of the element size.  Slots, level rules and geometry
 * are those of dwt_hip_bands_apply_batch: 3J + 1 slots, HL, LH, HH of level 1 .. J and then LL(J), J =
 * dwt_hip_band_levels(size_x, size_y, j_max) with j_max the count the forward transform returned, the rectangles those
 * of dwt_hip_band_geometry.  `steps` is a HOST array with one step per slot; table_stride 0: one table for all frames,
 * otherwise frame b reads steps + b*table_stride (at least the slot count).
 *
 * Quantize.  Per slot inv = 1.0f / step, an IEEE binary32 division made on the host.  Per sample c (binary16 widened
 * to binary32 first, exactly): m = fabsf(c) * inv, ONE rounded product; k = (int)m by truncation, with NaN giving 0 and
 * m >= 32768.0f (int16) or m >= 2147483648.0f (int32) giving 32767 or 2147483647 -- both cases count as CLIPPED; the index
 * is -k where the sign bit of c is set and k otherwise, so -0.0f and everything inside the deadzone give 0.
 *
 * Dequantize.  q == 0 gives +0.0f.  Otherwise a = (float)|q|, the magnitude taken so that INT32_MIN gives 2147483648.0f;
 * v = (a + r) * step, a rounded sum and a rounded product (never contracted); the sign of q is applied to v; a binary16
 * destination rounds v once more, to nearest even.  r in [0, 1) is the reconstruction offset: with r = 0.5 (or any r that
 * keeps (a + r) * step inside the index's cell) quantizing the result returns q; r = 0 is legal but puts the value on the
 * cell's edge, where the product's rounding decides.
 *
 * `stats` (quantize; HOST memory, may be NULL): {nonzero indices, largest magnitude k, clipped samples} as three long
 * long per slot per frame, frame b's at stats + 3*slots*b.  Summed with integer atomics only: every run gives the same
 * values.  The magnitude bit-planes of a band are the bit length of its largest magnitude.
 *
 * dwt_hip_quant_norms (host code, no device): norm_l[j-1] and norm_h[j-1], j = 1 .. levels <= 16, the L2 norms of this
 * library's 1-D synthesis functions: a 1 at coefficient 32 of the 64 L (resp. H) coefficients of level j of a line of
 * 64 << j samples, every other coefficient 0, inverted j levels in double with the wavelet's binary32 constants widened
 * (the scaling factors as the float kernels form them), the root of the sum of the squares.  DWT_HIP_CDF97_S (use it for
 * _CDF97_H too), _CDF53_S and _INTERP53_S; any other wavelet is an error.
 * dwt_hip_quant_steps (host code): steps[slot] = (float)((double)base_step / (n_x * n_y)) for the 3*levels + 1 slots,
 * HL(j): n_x = norm_h[j], n_y = norm_l[j]; LH(j): n_x = norm_l[j], n_y = norm_h[j]; HH(j): both norm_h[j]; LL: both
 * norm_l[levels].  levels 0 .. 16, base_step finite and > 0.  Both return 0, or nonzero with dwt_hip_last_error.
 *
 * Code-blocks.  A band is cut into blocks of 2^cb_log2_x x 2^cb_log2_y samples (each exponent 2 .. 10, their sum at most
 * 12), anchored at the band's first sample, partial blocks at the right and at the bottom.  dwt_hip_codeblock_layout fills
 * first[0 .. slots] (the prefix of the slots' block counts, the last entry the total) and blocks_x[0 .. slots-1] (blocks
 * across; either may be NULL) and returns the total, -1 for bad arguments; an empty band has no blocks.
 * dwt_hip_codeblock_bitplanes_batch stores planes[b*planes_frame_stride + first[slot] + by*blocks_x[slot] + bx] = the bit
 * length (0 .. 32) of the largest |q| of block (bx, by): 0 for a block of zeros, 32 for one that holds INT32_MIN.  `planes`
 * is host or device memory, planes_frame_stride at least the total (the bytes between the frames' maps are left alone).
 * Index planes whose base, row pitch and batch stride are multiples of 16 bytes are read by whole aligned 16-byte chunks
 * (option "quant_wide" = 0: element by element, like every other plane; same bytes out): the chunk that holds the last
 * element of the last row is read whole, up to 15 bytes past that element inside the same aligned 16 bytes -- read, never
 * used, never written.
 *
 * Each of coef, index and planes is host or device memory on its own.  Device sides are ordered on the context's stream:
 * ONE kernel launch for the whole batch and the whole table (the tables cross in one small copy), no allocation after
 * the first call of a size; a call on device memory without `stats` does not wait for the device.  A host side is mirrored
 * in a device buffer of the context (a written region with bytes outside the frames is uploaded first, so that they come
 * back as they were) and the call ends synchronised, and so does every call with `stats`.  Only the frames' own elements
 * are written.  A lane moves a run of 16 / (the smaller element size) samples of a row; a side whose base, row pitch and
 * batch stride are multiples of 16 bytes moves by 16-byte accesses, any other side element by element (option
 * "quant_wide" = 0: every side): same bits.  dwt_hip_quant_route tells which: the OR of DWT_HIP_QUANT_WIDE_COEF and
 * _WIDE_INDEX for a call with these addresses (either direction), -1 for arguments the entries refuse; it holds for device
 * sides (a host side runs on its mirror, which is aligned).
 * In place: binary32 <-> int32 with coef == index and equal pitches and batch strides IS supported, in both directions
 * (a lane reads its run before it writes it).  Every other contact is refused: the two regions, from the first frame's
 * first byte to the last frame's last, must not share a byte.
 * Errors (nonzero, dwt_hip_last_error, nothing launched, nothing written): a step that is not finite or not > 0, r outside
 * [0, 1), a null pointer, negative sizes, a pitch below its row, frames closer than they span, addresses or strides that
 * are no multiple of the element size, unknown types, `stats` in device memory, regions that overlap. */
enum dwt_hip_coef_type { DWT_HIP_COEF_S = 0, DWT_HIP_COEF_H = 1 };
enum dwt_hip_index_type { DWT_HIP_INDEX_I16 = 0, DWT_HIP_INDEX_I32 = 1 };
#define DWT_HIP_QUANT_MAX_LEVELS 16 /* of dwt_hip_quant_norms / _steps */
#define DWT_HIP_QUANT_GRID_ROWS 16384 /* rows / frames one trip of the quantizer's loops covers */
#define DWT_HIP_QUANT_GRID_BATCH 4096
#define DWT_HIP_CODEBLOCK_GRID_BLOCKS 65536 /* code-blocks one trip of the bit-plane kernel's loop covers */
#define DWT_HIP_QUANT_WIDE_COEF 1
#define DWT_HIP_QUANT_WIDE_INDEX 2
int dwt_hip_quant_norms(int wavelet, int levels, double *norm_l, double *norm_h);
int dwt_hip_quant_steps(int wavelet, int levels, float base_step, float *steps);
int dwt_hip_quantize_batch(int coef_type, const void *coef, size_t coef_batch_stride, size_t coef_row_pitch, int index_type,
	void *index, size_t index_batch_stride, size_t index_row_pitch, int batch, int size_x, int size_y, int j_max,
	const float *steps, size_t table_stride, long long *stats);
int dwt_hip_dequantize_batch(int index_type, const void *index, size_t index_batch_stride, size_t index_row_pitch, int coef_type,
	void *coef, size_t coef_batch_stride, size_t coef_row_pitch, int batch, int size_x, int size_y, int j_max,
	const float *steps, size_t table_stride, float r);
int dwt_hip_quant_route(int coef_type, const void *coef, size_t coef_batch_stride, size_t coef_row_pitch, int index_type,
	const void *index, size_t index_batch_stride, size_t index_row_pitch, int batch, int size_x, int size_y);
int dwt_hip_codeblock_layout(int size_x, int size_y, int j_max, int cb_log2_x, int cb_log2_y, int *first, int *blocks_x);
int dwt_hip_codeblock_bitplanes_batch(int index_type, const void *index, size_t index_batch_stride, size_t index_row_pitch,
	int batch, int size_x, int size_y, int j_max, int cb_log2_x, int cb_log2_y, unsigned char *planes,
	size_t planes_frame_stride);

/* Sparse coefficient streams: the nonzero elements of coefficient or index planes packed on the device
 * into (position, value) pairs in a fixed order, and scattered back.  What keep_largest_batch and quantize_batch leave is
 * almost all zeros; a coder, a store or a peer on the host wants the nonzeros, and only they need to cross PCIe.  An
 * extension: the reference has nothing of the kind; this comment is the specification (tests/sparse_model.py restates it
 * in numpy, the device is held to it bit for bit -- there is no arithmetic and no tolerance).
 *
 * Frames.  `batch` dense Mallat frames of size_x x size_y elements of `type` (DWT_HIP_SPARSE_F32, _F16, _I16, _I32; 4, 2,
 * 2, 4 bytes), element (x, y) of frame b at planes + b*batch_stride + y*row_pitch + x*(element size) bytes; J =
 * dwt_hip_band_levels(size_x, size_y, j_max) levels and the 3J + 1 slots of dwt_hip_band_geometry, j_max as the band
 * operators take it.
 *
 * Kept elements.  An integer element is kept when it is not 0 (INT16_MIN and INT32_MIN are kept).  A float element is
 * kept when its bits with the sign bit cleared are not 0: NaN, Inf and subnormals are kept with their bits; +0.0 and -0.0
 * are dropped.  Unpack writes zero BITS where there is no entry, so a -0.0 comes back as +0.0: the one place where a
 * round trip changes bits.
 *
 * Stream order (resolution order).  Bands coarse to fine: slot 3J (LL) first, then the three slots of level J in slot
 * order (HL, LH, HH), then level J-1, ... down to level 1; inside a band raster order, rows top to bottom, each row left
 * to right.  Empty bands contribute nothing.  A prefix of a stream is a coarser picture.  dwt_hip_sparse_order (host
 * code, no device) stores the 3*levels + 1 slot numbers in stream order and returns their count (-1: levels outside
 * 0 .. 31 or a null pointer).
 *
 * An entry is a position and a value in two separate dense arrays: pos[i] = y*size_x + x, a uint32 in frame coordinates
 * whatever the pitch; val[i] the element's own bits, in the source type.  Frame b's entries start at element
 * b*stream_stride of each array; stream_stride is the per-frame capacity in entries.  A frame with more kept elements
 * than stream_stride gets its FIRST stream_stride entries in stream order; the others are not written.  That is no error:
 * a call on device memory does not wait for the device.
 * Offsets: uint32, 3J + 2 per frame, frame b's at offsets + b*(3J + 2): off[k] the number of entries in front of stream
 * band k (k in stream order), off[3J + 1] the frame's total -- always the true counts, whatever the capacity.
 *
 * dwt_hip_sparse_pack_batch.  pos == NULL && val == NULL (stream_stride ignored): count only, the sizing call.  `planes`
 * is only read.  Entries behind a frame's total, and the bytes between the frames' entries, are left alone.
 * dwt_hip_sparse_unpack_batch writes EVERY own element of every frame: the entry's value where there is one, zero bits
 * elsewhere; the bytes between a row's end and its pitch and between the frames are left alone.  Frame b has
 * min(counts[b*counts_stride], stream_stride) entries (counts: uint32; offsets + 3J + 1 with counts_stride 3J + 2 reads
 * pack's totals where they lie).  An entry whose pos >= size_x*size_y is skipped and never written.  The streams pack
 * produces hold no position twice; for a foreign stream that does, which entry wins is unspecified.
 *
 * Memory.  Three sides -- the planes, the stream (pos and val), the offsets / counts -- each in host or in device memory
 * on its own.  Device sides are ordered on the context's stream; with all three on the device no call waits for the
 * device, and after the first call of a size none allocates.  A host side is mirrored in scratch of the context (a
 * written region is uploaded first, so that the bytes the call leaves alone come back as they were) and the call ends
 * synchronised.
 * Kernels.  Pack is THREE launches whatever the batch, the shape and the density: the frames are cut into tiles of
 * DWT_HIP_SPARSE_TILE_SAMPLES consecutive samples of one band's raster order, enumerated in stream order
 * (dwt_hip_sparse_bands / _tile below); launch 1 counts every tile's kept elements, launch 2 -- one workgroup per frame --
 * turns the counts into the tiles' first entries and the frame's offsets, launch 3 reads the tiles again and writes every
 * entry at its tile's base plus its rank in the tile.  Count only is launches 1 and 2.  Unpack is TWO launches: the zero
 * fill, the scatter.  The order is fixed by construction: no atomics, no workgroup waits for another.  A lane reads runs
 * of 16 / (element size) consecutive samples of a row, by one 16-byte access where the planes' base, row pitch and batch
 * stride are multiples of 16 bytes and the run lies inside the row, element by element elsewhere (option "sparse_wide" =
 * 0: everywhere); same bits.  dwt_hip_sparse_route: 1 where a call with these addresses takes the 16-byte route, 0 where
 * not, -1 for arguments the entries refuse (it holds for device planes; host planes run on their aligned mirror).
 * batch == 0 launches nothing and writes nothing; frames without elements launch nothing, their offsets are written as
 * zeros.
 * Errors (nonzero, dwt_hip_last_error, nothing launched, nothing written): a null pointer other than the count-only pair,
 * val without pos or pos without val, an unknown type, negative sizes, size_x*size_y > INT_MAX, a pitch below its row,
 * frames closer than they span, addresses or strides that are no multiple of the element size (4 for pos, offsets and
 * counts), regions that share a byte (the planes with the stream, the offsets or the counts; the stream's arrays and the
 * offsets with each other).
 *
 * dwt_hip_sparse_bands (host code): {x, y, size_x, size_y, first tile} of every band in STREAM order -> table, five ints
 * per band, and one more row {0, 0, 0, 0, tiles of a frame}; 5 * (3J + 2) ints in all.  Returns 3J + 1, -1 for sizes the
 * entries refuse.  dwt_hip_sparse_tile: tile `tile` of that table -> its band (stream order), its first sample in the
 * band's raster order and its sample count; 0, or -1 for a tile the table does not hold. */
enum dwt_hip_sparse_type { DWT_HIP_SPARSE_F32 = 0, DWT_HIP_SPARSE_F16 = 1, DWT_HIP_SPARSE_I16 = 2, DWT_HIP_SPARSE_I32 = 3 };
#define DWT_HIP_SPARSE_TILE_SAMPLES 2048 /* samples of a tile */
#define DWT_HIP_SPARSE_GRID_TILES 4096 /* tiles / frames one trip of the kernels' loops covers */
#define DWT_HIP_SPARSE_GRID_BATCH 4096
int dwt_hip_sparse_order(int levels, int *slots);
int dwt_hip_sparse_bands(int size_x, int size_y, int j_max, int *table);
int dwt_hip_sparse_tile(const int *table, int bands, int tile, int *band, int *start, int *count);
int dwt_hip_sparse_pack_batch(int type, const void *planes, size_t batch_stride, size_t row_pitch, int batch, int size_x, int size_y,
	int j_max, unsigned *pos, void *val, size_t stream_stride, unsigned *offsets);
int dwt_hip_sparse_unpack_batch(int type, const unsigned *pos, const void *val, size_t stream_stride, const unsigned *counts,
	size_t counts_stride, void *planes, size_t batch_stride, size_t row_pitch, int batch, int size_x, int size_y);
int dwt_hip_sparse_route(int type, const void *planes, size_t batch_stride, size_t row_pitch, int batch, int size_x, int size_y);

/* Embedded bit-plane streams of code-blocks: the code-blocks of index planes packed on the device into a
 * sign plane and as many magnitude planes as the block's largest magnitude has bits, and unpacked again, with the least
 * significant planes left out on request.  Where 5 % to 100 % of the indices are nonzero -- every visually useful step --
 * the sparse streams cost more than the planes themselves; a block whose largest magnitude has p bits needs p + 1 bits a
 * sample, a block of zeros nothing.  An extension: the reference has nothing of the kind; this comment is the
 * specification (tests/bitplane_model.py restates it in numpy, the device is held to it bit for bit -- there is no
 * arithmetic and no tolerance).
 *
 * Frames.  `batch` index planes of size_x x size_y elements of `index_type` (DWT_HIP_INDEX_I16, _I32), element (x, y) of
 * frame b at index + b*batch_stride + y*row_pitch + x*(element size) bytes: the addressing of the quantizer's index side,
 * base and strides multiples of the element size.
 *
 * Blocks.  The code-blocks of dwt_hip_codeblock_layout(size_x, size_y, j_max, cb_log2_x, cb_log2_y, ...): each exponent
 * 2 .. 10, their sum at most 12, so that a block holds at most 4096 samples.  Blocks are enumerated in STREAM ORDER: the
 * bands in the order of dwt_hip_sparse_order (LL, then HL, LH, HH of level J, ... down to level 1), inside a band the
 * blocks in raster order.  S is the number of blocks of a frame.  A block of cw x ch samples (partial blocks at the right
 * and at the bottom keep their own width) has n = cw*ch samples; sample i is the one at column i % cw, row i / cw of the
 * block; G = ceil(n / 64).
 *
 * A block's words.  p is the bit length (0 .. 32) of the block's largest |q| -- the value
 * dwt_hip_codeblock_bitplanes_batch stores; INT16_MIN gives 16, INT32_MIN 32.  p == 0: no words.  Otherwise the block
 * holds (p + 1)*G 64-bit words (uint64_t, native byte order), plane-major: plane 0 is the sign plane (bit set where
 * q < 0), plane k = 1 .. p is bit p - k of |q|, most significant first.  Inside a plane word g holds samples 64g .. 64g +
 * 63, sample 64g + i in bit i (bit 0 the least significant); bits past sample n - 1 are 0.
 * The stream is EMBEDDED: a prefix of a block's planes is the same block at a coarser step, a prefix of the blocks in
 * stream order a coarser picture.
 *
 * A frame's stream.  Frame b's words start at words + b*stream_stride (counted in words), the blocks in stream order
 * without gaps.  Offsets: uint32, S + 1 per frame, frame b's at offsets + b*(S + 1): off[s] the number of words in front
 * of block s, off[S] the frame's total -- always the true sizes, whatever the capacity.  p is not stored:
 * (off[s+1] - off[s]) / G - 1 is p.
 * Capacity.  Block s is written only if off[s+1] <= stream_stride; later blocks are not written, and the words behind the
 * last written block are left alone.  That is no error: a call on device memory does not wait for the device.
 *
 * dwt_hip_bitplane_pack_batch.  words == NULL (stream_stride ignored): count only, the sizing call.  `index` is only read.
 * dwt_hip_bitplane_unpack_batch writes EVERY own element of every frame and nothing else.  drop in 0 .. 32: the
 * min(drop, p) least significant magnitude planes of every block are not read.  With m = |q| >> min(drop, p) taken from
 * the planes that are read, mode DWT_HIP_BITPLANE_KEEP stores the magnitude m << min(drop, p) (the element keeps its
 * step), DWT_HIP_BITPLANE_SHIFT stores m (the caller dequantizes with steps * 2^drop and r = 0.5, the midpoint of the
 * coarser cell).  A magnitude of 0 stores 0 whatever the sign bit; otherwise the sign plane negates the magnitude.  The
 * value is stored truncated to the element type: INT16_MIN and INT32_MIN come back, a foreign stream's oversized magnitude
 * wraps.
 * Foreign and cut streams.  Unpack never reads a word outside [frame base, frame base + stream_stride) and never an
 * offset outside the frame's S + 1.  A block is written as zeros when off[s+1] < off[s], when off[s+1] > stream_stride,
 * when off[s+1] - off[s] is no multiple of G, or when its p exceeds 16 (int16) / 32 (int32).  That is also how a stream
 * cut by pack's capacity comes back: a prefix of the blocks, zeros for the rest.
 *
 * Memory.  Three sides -- the planes, the words, the offsets -- each in host or in device memory on its own.  Device
 * sides are ordered on the context's stream; with all three on the device no call waits for the device, and after the
 * first call of a size none allocates.  A host side is mirrored in scratch of the context (a written region is uploaded
 * first, so that the bytes the call leaves alone come back as they were) and the call ends synchronised.
 * Kernels.  Pack is THREE launches whatever the batch, the shape and the content: launch 1 reads every block's largest
 * magnitude (a wave per block; the reading code of dwt_hip_codeblock_bitplanes_batch with its 16-byte route, option
 * "quant_wide") and stores the block's size, launch 2 -- one workgroup per frame -- turns the sizes into the offsets,
 * launch 3 -- a workgroup per block, DWT_HIP_BITPLANE_GRID_BLOCKS of them per trip of its loop -- reads the block again, a
 * wave per group of 64 samples, builds each plane's word by one 64-bit ballot, assembles the words in LDS and stores them
 * as one run.  Count only is launches 1 and 2.  Unpack is ONE launch: the planes that are read go contiguously into LDS
 * (dropped planes cost no bytes) and every element of every block is written, by 16-byte runs of a row where the planes'
 * base, row pitch and batch stride and the block's first column are multiples of 16 bytes, element by element elsewhere;
 * same bytes.  No atomics, no workgroup waits for another.
 * Option "bitplane_wave" = 0: launch 3 and unpack take a plain route, one lane per word touching its 64 samples itself --
 * same bytes, the on-device cross-check.  dwt_hip_bitplane_route: 1 where a call with these arguments runs the wave
 * kernels, 0 for the cross-check route, -1 for arguments the entries refuse.
 * batch == 0 launches nothing and writes nothing; frames without elements launch nothing, their offsets are written as
 * zeros.
 * Errors (nonzero, dwt_hip_last_error, nothing launched, nothing written): a null pointer other than `words` of the
 * count-only call, an unknown type or mode, drop outside 0 .. 32, bad exponents, negative sizes, size_x*size_y > INT_MAX, a
 * pitch below its row, frames closer than they span, addresses or strides that are no multiple of the element size (8 for
 * words, 4 for offsets), regions that share a byte.
 *
 * Host geometry (no device).  dwt_hip_bitplane_bands: {x, y, size_x, size_y, first stream block} of every band in stream
 * order -> table, five ints per band, and one more row {0, 0, 0, 0, S}; 5 * (3J + 2) ints in all.  Returns 3J + 1, -1 for
 * arguments the entries refuse.  dwt_hip_bitplane_block: stream block s of that table -> its rectangle in frame
 * coordinates; 0, or -1 for a block the table does not hold.  dwt_hip_bitplane_words: the size rule, (p + 1) * ceil(n / 64)
 * words for p > 0, 0 for p == 0; -1 for n outside 1 .. 4096 or p outside 0 .. 32. */
#define DWT_HIP_BITPLANE_KEEP 0
#define DWT_HIP_BITPLANE_SHIFT 1
#define DWT_HIP_BITPLANE_GRID_BLOCKS 16384 /* code-blocks one trip of the pack / unpack kernels' loops covers */
#define DWT_HIP_BITPLANE_GRID_BATCH 4096 /* frames one trip of the scan's loop covers */
int dwt_hip_bitplane_bands(int size_x, int size_y, int j_max, int cb_log2_x, int cb_log2_y, int *table);
int dwt_hip_bitplane_block(const int *table, int bands, int cb_log2_x, int cb_log2_y, int s, int *x, int *y, int *w, int *h);
int dwt_hip_bitplane_words(int n, int p);
int dwt_hip_bitplane_pack_batch(int index_type, const void *index, size_t batch_stride, size_t row_pitch, int batch, int size_x,
	int size_y, int j_max, int cb_log2_x, int cb_log2_y, uint64_t *words, size_t stream_stride, unsigned *offsets);
int dwt_hip_bitplane_unpack_batch(int index_type, const uint64_t *words, size_t stream_stride, const unsigned *offsets, void *index,
	size_t batch_stride, size_t row_pitch, int batch, int size_x, int size_y, int j_max, int cb_log2_x, int cb_log2_y, int drop, int mode);
int dwt_hip_bitplane_route(int index_type, const void *index, size_t batch_stride, size_t row_pitch, int batch, int size_x, int size_y,
	int j_max, int cb_log2_x, int cb_log2_y);

/* User-defined lifting wavelets: a multi-level Mallat transform of a batch of dense frames by a lifting
 * scheme that the CALLER describes in a small table -- Haar, Daubechies D4, 13/7, 2/6, the S transform, a filter of one's
 * own --, binary32 or reversible int32.  An extension: the reference has Haar and D4 as cores only (examples/cores/
 * cores-haar.c, cores-d4.c); this comment is the specification, tests/lifting_model.py restates it in numpy, and the
 * device is held to it bit for bit.  The planes are plain Mallat planes (dwt_hip_band_levels / dwt_hip_band_geometry), so
 * the band operators, the quantizer, the sparse streams, the N-term selection and the feature statistics take them.
 *
 * The scheme (struct dwt_hip_lifting: fixed size, no pointers).  `type` DWT_HIP_LIFT_F32 (binary32 samples) or
 * DWT_HIP_LIFT_I32 (int32 samples).  `n_steps` 1 .. 8 steps; a step updates the samples of one `parity` of a line (1: the
 * odd ones, 0: the even ones; consecutive steps may share a parity) from `n_terms` 1 .. 4 terms.  A term has two tap offsets
 * relative to the target sample: off_a odd, -7 .. 7; off_b odd, -7 .. 7, or 0 for "no second tap".  A step therefore reads
 * only the other parity and runs in place without a race.
 *   float step:  t_k = coef_k * (x[i+off_a] + x[i+off_b]), or coef_k * x[i+off_a] for a single tap;
 *                sum = ((t_0 + t_1) + t_2) + t_3 over the terms there are; x[i] = x[i] + sum forward, x[i] - sum inverse.
 *                Every product and every sum is rounded on its own (no FMA).  coef finite.  num, sign, add, shift unused.
 *   int step:    v = (SUM_k num_k * (a_k + b_k) + add) >> shift (b_k absent for a single tap), wrapping 32-bit arithmetic,
 *                arithmetic shift, shift 0 .. 31; x[i] += sign * v forward, x[i] -= sign * v inverse; sign +1 or -1.
 *                coef unused.
 * Scaling, float only, indexed by parity: forward, after the last step, x *= fwd_scale[parity]; inverse, first x *=
 * inv_scale[parity], then the steps last to first.  All four values are explicit (CDF 9/7's 1.0f / zeta and (float)(1 /
 * zeta) are different floats) and finite; a factor of exactly 1.0f is skipped.  Int schemes do not scale.
 * A 2-D level: the forward lifts every row, then every column.  The inverse lifts rows, then columns when
 * inverse_cols_first is 0 (the order of the reference's float drivers) and columns, then rows when it is 1 (the exact
 * mirror).  Int schemes must say 1: they are then reversible bit for bit, wrapped values included.
 * Line ends: whole-sample symmetric reflection of the INDEX of every tap, at every step, into [0, N): i < 0 -> -i,
 * i > N-1 -> 2(N-1) - i, repeated until it lies inside (lines shorter than the reach bounce more than once).  Reflection
 * keeps parity, so every scheme is invertible whatever its taps.  A line of ONE sample runs no step: it is only scaled by
 * the factor of parity 0 (float) or left as it is (int).
 * The reach of a scheme is R = the sum over its steps of the largest |offset| of the step.
 *
 * dwt_hip_lifting_check (host code, no device): 0 for a scheme that holds to all of the above, and *reach = R (reach may
 * be NULL); nonzero with dwt_hip_last_error for any other.  dwt_hip_lifting_builtin (host code): the scheme of `id` ->
 * *scheme, 0; nonzero for an unknown id.  CDF97, CDF53, INTERP53 (float) and CDF53_INT, CDF97_INT give the bits of
 * DWT_HIP_CDF97_S, _CDF53_S, _INTERP53_S, _CDF53_I, _CDF97_I wherever a line has two samples or more and no doubled
 * end tap overflows (|x| <= FLT_MAX / 2; int 5/3: |x| < 2^30).  HAAR: odd += -1 x[i-1], even += 0.5 x[i+1], scales 1 (the
 * reference's element step).  HAAR_INT, the S transform: odd -= x[i-1], even += x[i+1] >> 1.  D4: the reference's
 * factorization, odd += alpha x[i+1]; even += beta x[i-1] + gamma x[i+1]; odd += delta x[i-1]; alpha = -1/sqrt 3, beta =
 * (6 - 3 sqrt 3)/4, gamma = sqrt 3 / 4, delta = -1/3, scales (3 +- sqrt 3)/(3 sqrt 2) forward and their own reciprocal
 * expressions inverse, each the float the reference's expression yields (tests/golden/lifting.npz).
 *
 * dwt_hip_lifting2d_batch: `batch` dense frames (size_o == size_i) of size_x x size_y samples, element (x, y) of frame b
 * at base + b*batch_stride + y*stride_x + x*stride_y bytes, src -> dst (the same strides on both sides); src == dst is
 * allowed, any other overlap of the two is refused.  J = dwt_hip_band_levels(size_x, size_y, *j) levels, stored to *j;
 * level k acts on the ceil(size / 2^k) LL rectangle; L takes ceil(N/2) samples at offset 0, H floor(N/2) samples at offset
 * ceil(N/2).  `scheme` is host memory, copied at the call.  src / dst are host or device memory, both the same; dense
 * device frames (stride_y == 4, addresses and strides multiples of 4 bytes) run where they lie and the call does not
 * wait for the device; host and strided frames go through the staging path and end synchronised.
 * Routes.  FUSED (R <= 8): ONE launch per level for the whole batch -- a workgroup owns a 64 x 64 tile of the level, stages
 * it with a halo of R samples in LDS, runs the row steps and the column steps in place there (the halo is recomputed, never
 * exchanged; positions outside the frame are never lifted: every tap reflects its index and reads the cell of the sample it
 * lands on), scales and writes the four subbands; LL goes through scratch of the context.  src == dst costs one more
 * launch and a copy of the batch in scratch (the tiles read halos that other tiles overwrite).  STEPS (option
 * "lifting_fused" = 0, and R > 8): per level one copy of the LL rectangle into dense scratch, one elementwise launch per
 * step and direction, one launch that scales and places the subbands.  Same bits.  dwt_hip_lifting_route: DWT_HIP_LIFT_FUSED
 * or DWT_HIP_LIFT_STEPS for a call with this scheme under the current options, -1 for a scheme the entries refuse.
 * Errors (nonzero, dwt_hip_last_error, nothing launched, nothing written): a bad scheme, a null pointer, sizes < 1, batch
 * < 1 or > DWT_HIP_LIFT_MAX_BATCH, strides below the element, a row or a frame, src and dst in different memory spaces or
 * overlapping. */
enum dwt_hip_lifting_type { DWT_HIP_LIFT_F32 = 0, DWT_HIP_LIFT_I32 = 1 };
enum dwt_hip_lifting_id {
	DWT_HIP_LIFT_CDF97 = 0, DWT_HIP_LIFT_CDF53, DWT_HIP_LIFT_INTERP53, DWT_HIP_LIFT_CDF53_INT, DWT_HIP_LIFT_CDF97_INT,
	DWT_HIP_LIFT_HAAR, DWT_HIP_LIFT_HAAR_INT, DWT_HIP_LIFT_D4
};
enum dwt_hip_lifting_route_id { DWT_HIP_LIFT_STEPS = 0, DWT_HIP_LIFT_FUSED = 1 };
#define DWT_HIP_LIFT_MAX_STEPS 8
#define DWT_HIP_LIFT_MAX_TERMS 4
#define DWT_HIP_LIFT_MAX_OFFSET 7
#define DWT_HIP_LIFT_FUSED_REACH 8 /* the largest reach the fused route takes */
#define DWT_HIP_LIFT_MAX_BATCH 65535 /* frames of one call (the tile kernels' grid.z) */
struct dwt_hip_lifting_term {
	float coef;       /* float schemes */
	int num;          /* int schemes */
	int off_a, off_b; /* tap offsets; off_b 0: no second tap */
};
struct dwt_hip_lifting_step {
	int parity, n_terms;
	int sign, add, shift; /* int schemes */
	int reserved[3];      /* 0 */
	struct dwt_hip_lifting_term terms[DWT_HIP_LIFT_MAX_TERMS];
};
struct dwt_hip_lifting {
	int type, n_steps, inverse_cols_first;
	int reserved; /* 0 */
	float fwd_scale[2], inv_scale[2];
	struct dwt_hip_lifting_step steps[DWT_HIP_LIFT_MAX_STEPS];
}; /* 800 bytes */
int dwt_hip_lifting_check(const struct dwt_hip_lifting *scheme, int *reach);
int dwt_hip_lifting_builtin(int id, struct dwt_hip_lifting *scheme);
int dwt_hip_lifting2d_batch(const struct dwt_hip_lifting *scheme, int inverse, const void *src, void *dst, size_t batch_stride,
	int batch, int stride_x, int stride_y, int size_x, int size_y, int *j);
int dwt_hip_lifting_route(const struct dwt_hip_lifting *scheme);

/* User-defined lifting wavelets of LINE batches, and the quantizer norms of a scheme.  An extension like
 * the one above; this comment is the specification, tests/lifting1d_model.py restates it in numpy (on the line pass of
 * tests/lifting_model.py), and the device is held to it bit for bit.
 *
 * dwt_hip_lifting1d_batch: `n_lines` dense lines (size_o == size_i) of `size` samples, element i of line n at base +
 * n*line_stride + i*elem_stride bytes, src -> dst with the same strides on both sides.  The result is the multi-level 1-D
 * Mallat layout of dwt_hip_transform1d_batch: level k acts on the first ceil(size / 2^k) samples of every line; L takes
 * ceil(n/2) samples at offset 0, H floor(n/2) samples at offset ceil(n/2).  So dwt_hip_features1d_batch, the packet and
 * the conditioning entries take the lines as they are.
 * Levels.  With limit = ceil_log2(size): forward, a *j outside 0 .. limit becomes the limit, and the count used is stored
 * to *j; inverse, a *j inside 0 .. limit - 1 is used as it is, any other value stands for the limit, and *j is only read.
 * (Both as dwt_hip_transform1d_batch does it.)  No level: the lines are copied, or left alone when src == dst.
 * One level of one line is the line pass of the 2-D specification above, unchanged: the scheme's steps first to last,
 * every tap reflecting its INDEX into [0, n) bounce by bounce, then x *= fwd_scale[parity]; the inverse applies
 * inv_scale[parity] first, then the steps last to first, float schemes subtracting the sum and int schemes sign * v.  A line
 * of one sample runs no step and is only scaled by the factor of parity 0.  inverse_cols_first has no meaning here (and
 * dwt_hip_lifting_check still asks int schemes to say 1).
 * src == dst is allowed (a line is read whole before any of it is written); any other overlap of the two is refused.
 * Memory.  src and dst are both host or both device memory.  Device lines whose addresses and strides are multiples of 4
 * bytes run where they lie -- any such elem_stride, so one channel of interleaved data does -- and the call does not wait
 * for the device.  Host memory and every other device layout go through the staging path and end synchronised.
 * Routes.  FUSED: every level whose input line has at most 8192 samples runs in ONE launch for the whole batch, whatever
 * the depth and whatever the scheme's reach -- the line lies in LDS whole, so there is no halo and no reach limit.  STEPS
 * (option "lifting_fused" = 0, and the leading levels of lines longer than 8192 samples): per level the lines' prefix is
 * copied into dense scratch, every step is one elementwise launch there, and one launch scales and places the result; a
 * longer line runs its over-long levels this way and the rest in one fused launch.  Same bits.  dwt_hip_lifting1d_route:
 * DWT_HIP_LIFT_FUSED where a call with this scheme and this size runs in one launch under the current options,
 * DWT_HIP_LIFT_STEPS where not, -1 for a scheme or a size the entry refuses.
 * Errors (nonzero, dwt_hip_last_error, nothing launched, nothing written): a bad scheme, a null pointer, size < 1, n_lines
 * < 1, an elem_stride below 4, a line_stride below what a line spans, src and dst in different memory spaces or overlapping.
 *
 * dwt_hip_lifting_norms (host code, no device; float schemes only): norm_l[j-1] and norm_h[j-1], j = 1 .. levels <=
 * DWT_HIP_QUANT_MAX_LEVELS, the L2 norms of the scheme's 1-D synthesis functions: a 1 at the middle L (resp. H) coefficient
 * of level j, every other coefficient 0, inverted j levels in double -- inv_scale first, the steps last to first, coef * (a
 * + b) and ((t0 + t1) + t2) + t3 evaluated in double on the binary32 constants widened --, the root of the sum of the
 * squares.  The line is sized from the scheme's reach (4 (R + 2) << (j - 1) samples) so that no tap reflects.  With the
 * CDF97, CDF53 and INTERP53 tables this is dwt_hip_quant_norms of the wavelet.
 * dwt_hip_lifting_quant_steps (host code): the 3*levels + 1 steps of dwt_hip_quant_steps, by its formula, from those
 * norms; the table goes to dwt_hip_quantize_batch as it is.  levels 0 .. 16, base_step finite and > 0.
 * Both return 0, or nonzero with dwt_hip_last_error: a bad or an int scheme, a null pointer, levels out of range, a bad base
 * step. */
int dwt_hip_lifting1d_batch(const struct dwt_hip_lifting *scheme, int inverse, const void *src, void *dst, size_t line_stride,
	int elem_stride, int n_lines, int size, int *j);
int dwt_hip_lifting1d_route(const struct dwt_hip_lifting *scheme, int size);
int dwt_hip_lifting_norms(const struct dwt_hip_lifting *scheme, int levels, double *norm_l, double *norm_h);
int dwt_hip_lifting_quant_steps(const struct dwt_hip_lifting *scheme, int levels, float base_step, float *steps);

/* Time-frequency planes of line batches: the Gaussian-window STFT, the complex Morlet CWT and the S transform of
 * src/gabor.c (gabor_ft_s, gabor_wt_s, gabor_st_s and their _arg_ twins; include/gabor.h), DESIGN.md s14.
 *
 * A BANK is `bins` complex kernels, each with its number of taps and its centre (0 <= centre < taps).  _bank_create
 * generates the kernels of one transform exactly as the reference does, in float with the host's libm: kind FT reads
 * sigma, WT reads sigma and freq, ST neither.  _bank_from_kernels takes them from the caller: sizes[bins],
 * centers[bins], and the taps of all kernels one after the other as (re, im) pairs.  Both return NULL on error
 * (dwt_hip_last_error) and need no device.  _bank_query copies sizes, centres and taps back (any pointer may be NULL;
 * the tap array holds 2 * dwt_hip_timefreq_bank_taps floats).  A bank is used by one thread at a time.
 *
 * dwt_hip_timefreq_batch correlates every line with every kernel: with x the line's N samples, k the kernel of bin y,
 *     c(t) = sum over i = -min(t, centre) .. min(N-1-t, taps-centre-1), ascending, of x[t+i] * conj(k[centre+i])
 * summed from +0 in float, every product and sum rounded on its own: bit-identical to dwt_util_cdot1_s.  Bin y writes
 * plane row bins-1-y, as the reference does.  out_kind DWT_HIP_TIMEFREQ_COMPLEX stores c as (re, im) pairs, _ABS the
 * magnitude (bit-identical to cabsf over the whole float range), _ARG the argument (atan2 in double, rounded once).
 * Output (line, row, t) goes to dst + line*plane_stride + row*row_stride + t*(8 for complex, else 4) bytes;
 * _batch_strided takes the distance of the row's elements as well.  Lines are line_stride bytes apart, their samples
 * elem_stride.  Both pointers are host memory or both device memory; they must not overlap (an error); n_lines, N and
 * bins are at least 1.  A call on device memory takes ONE kernel launch, whatever n_lines, bins and the kernel sizes;
 * kernels of any size are taken.  Option "timefreq_tiled" = 0 selects the plain kernel (one thread per output). */
typedef struct dwt_hip_timefreq_bank dwt_hip_timefreq_bank;
enum dwt_hip_timefreq_kind { DWT_HIP_TIMEFREQ_FT = 0, DWT_HIP_TIMEFREQ_WT = 1, DWT_HIP_TIMEFREQ_ST = 2 };
enum dwt_hip_timefreq_out { DWT_HIP_TIMEFREQ_COMPLEX = 0, DWT_HIP_TIMEFREQ_ABS = 1, DWT_HIP_TIMEFREQ_ARG = 2 };
dwt_hip_timefreq_bank *dwt_hip_timefreq_bank_create(int kind, int bins, float sigma, float freq);
dwt_hip_timefreq_bank *dwt_hip_timefreq_bank_from_kernels(int bins, const int *sizes, const int *centers, const float *taps);
void dwt_hip_timefreq_bank_free(dwt_hip_timefreq_bank *bank);
int dwt_hip_timefreq_bank_bins(const dwt_hip_timefreq_bank *bank);
long dwt_hip_timefreq_bank_taps(const dwt_hip_timefreq_bank *bank); /* of all kernels together */
int dwt_hip_timefreq_bank_query(const dwt_hip_timefreq_bank *bank, int *sizes, int *centers, float *taps);
int dwt_hip_timefreq_batch(dwt_hip_timefreq_bank *bank, const void *src, size_t line_stride, size_t elem_stride, int n_lines, int N,
	int out_kind, void *dst, size_t plane_stride, size_t row_stride);
int dwt_hip_timefreq_batch_strided(dwt_hip_timefreq_bank *bank, const void *src, size_t line_stride, size_t elem_stride, int n_lines,
	int N, int out_kind, void *dst, size_t plane_stride, size_t row_stride, size_t dst_elem_stride);
/* dwt_util_cdot1_s: the one sum c(func_center) of a signal (host or device) with one kernel of (re, im) pairs kern_stride
 * bytes apart (host); re_im[2] is host memory */
int dwt_hip_cdot1(const float *func, int func_size, int func_stride, int func_center, const float *kern, int kern_size,
	int kern_stride, int kern_center, float *re_im);
/* What include/gabor.h's entries stand on.  dwt_hip_gabor_transform: one plane of one signal as gabor_{ft,wt,st}[_arg]_s
 * takes it (`kind` as above, arg != 0 for the argument; plane element (row, t) at plane + row*stride_x + t*stride_y);
 * dwt_hip_timefreq_line: one line against one kernel of (re, im) pairs kern_stride bytes apart in host memory
 * (timefreq_line / timefreq_arg_line).  The generators run on the host: dwt_hip_gaussian_size = (int)ceilf(1 + 2 * 4 *
 * sigma * a), the centre is half of it; dwt_hip_gabor_wavelet stores gabor_wavelet(t, sigma, f, a) -- gabor_function
 * for a = 1 -- as re_im[2]; dwt_hip_gabor_gen_kernel writes the dwt_hip_gaussian_size(sigma, a) taps of
 * gabor_gen_kernel, `stride` bytes apart, into memory the caller holds. */
int dwt_hip_gabor_transform(int kind, int arg, const float *sig, int sig_stride, int sig_size, void *plane, int stride_x, int stride_y,
	int bins, float sigma, float freq);
int dwt_hip_timefreq_line(int arg, float *dst, int dst_stride, const float *src, int src_stride, int size, const void *kern,
	int kern_stride, int kern_size, int kern_center);
int dwt_hip_gaussian_size(float sigma, float a);
void dwt_hip_gabor_wavelet(float t, float sigma, float f, float a, float *re_im);
void dwt_hip_gabor_gen_kernel(void *kern, int stride, float sigma, float freq, float a);
/* The operators of src/gabor.c over a batch of planes: element (y, x) of plane p at base + p*plane_stride + y*stride_x +
 * x*stride_y bytes in the source and in the destination, which must not overlap; host or device memory alike.
 * dwt_hip_phase_derivative: phase_derivative_s, the difference of neighbouring angles along x wrapped by 2 pi into
 * [-limit, +limit], limit > 0 (a value the wrap step does not move -- the reference would not return -- is left).
 * dwt_hip_detect_ridges: detect_ridges1_s / 2_s / 3_s by `kind` 1 / 2 / 3.  Bit-identical to the reference, except that
 * kind 3 quantises the gradient direction with cos and sin taken in double (the reference: cosf, sinf): a point may
 * differ only where the cosine or sine of its gradient angle lies within a rounding error of +-1/2. */
int dwt_hip_phase_derivative(const void *angle, void *derivative, int stride_x, int stride_y, int size_x, int size_y, int n_planes,
	size_t plane_stride, float limit);
int dwt_hip_detect_ridges(int kind, const void *src, void *ridges, int stride_x, int stride_y, int size_x, int size_y, int n_planes,
	size_t plane_stride, float threshold);

/* ---- Windowed and reduced-resolution inverse 2-D transforms ----
 * A Mallat pyramid is a random-access format: a window of the reconstruction needs only the coefficients under it plus a
 * halo of K samples per level, and the frame at 1 / 2^r of its resolution -- LL(r) -- needs only the levels above r.
 *
 * Levels: J = ceil(log2(min(size_x, size_y))), cut by j_max when 0 <= j_max < J -- the count of the inverse 2-D drivers.
 * `discard` is r in 0 .. J.  The window [x0, x0 + w) x [y0, y0 + h) is in the coordinates of LL(r), a band of
 * Wo(r) x Ho(r) = ceil(size / 2^r) samples, and lies inside it with w, h >= 1.
 *
 * dwt_hip_window_regions: the rectangle of every subband that the window depends on, in elements from the frame's
 * origin, {x, y, size_x, size_y} per slot in the slot order of dwt_hip_band_geometry (3(l-1) + {0, 1, 2} = HL, LH, HH of
 * level l, slot 3J = LL(J)).  Returns 3J + 1, or -1 for arguments it refuses (a wavelet without a windowed inverse, sizes
 * below 1, discard outside 0 .. J, a window that is empty or leaves LL(r), a null table).  The slots of the discarded
 * levels l <= r hold {0, 0, 0, 0}; an empty rectangle has zero sizes.  Plain host arithmetic, no device.
 * The rule.  One line of N samples, the samples [a, b) wanted, K the wavelet's halo (4 for CDF 9/7, 2 for CDF 5/3 in
 * float, int32 and int16, 1 for the interpolating 5/3): a line of one sample needs L index 0 and no H; otherwise take the
 * interleaved indices 2 floor(a / 2) - K + 1 .. 2 floor((b - 1) / 2) + K + 1, fold each into [0, N) by whole-sample
 * reflection, let lo and hi be the least and the greatest folded index: L needs ceil(lo / 2) .. floor(hi / 2), H needs
 * floor(lo / 2) .. floor((hi - 1) / 2).  The levels: from X = [x0, x0 + w), Y = [y0, y0 + h), for l = r + 1 .. J,
 * (Lx, Hx) = need(X, Wo(l-1)), (Ly, Hy) = need(Y, Ho(l-1)); HL(l) is columns Wo(l) + Hx, rows Ly; LH(l) columns Lx, rows
 * Ho(l) + Hy; HH(l) columns Wo(l) + Hx, rows Ho(l) + Hy; then X = Lx, Y = Ly; LL(J) is X x Y.
 * The contract: dwt_hip_inverse_window_batch reads no element outside these rectangles -- a caller may upload only them
 * and leave the rest of the frame unwritten.
 *
 * dwt_hip_inverse_window_batch: `batch` dense Mallat frames in device memory, laid out as for dwt_hip_transform2d_batch
 * (frame b at src + b * batch_stride, rows stride_x bytes apart), only read.  Element (y, x) of destination frame b
 * (dst + b * dst_batch_stride, rows dst_stride_x bytes apart; y < h, x < w) is bit for bit element (y0 + y, x0 + x) of
 * dwt_hip_transform2d_batch(wavelet, 1, ...) at J - r levels on the top-left Wo(r) x Ho(r) rectangle of frame b; r == J
 * copies the window of LL(J).  Only those w x h elements of each destination frame are written; the destination takes any
 * base, pitch and batch stride that are multiples of the element size.
 * Wavelets: DWT_HIP_CDF97_S, _CDF53_S, _INTERP53_S, _CDF53_I, _CDF53_I16.  DWT_HIP_CDF97_H, _CDF97_I and the double
 * wavelets are out of scope: they are refused like any other id.
 * Routes, option "window_fused": 2 the window kernels wherever there is a level to undo -- one launch per level
 * l = J .. r + 1 for the whole batch, a workgroup per tile of DWT_HIP_WINDOW_TILE^2 samples of the level's region, the
 * halo recomputed per tile; 0 the cross-check, the inverse driver out of place into the context's scratch and a rectangle
 * copy (what a caller without this entry does); 1 (default) the kernels where they were measured to win -- a window of up
 * to 1 / 16 of LL(r) whose band, over the batch, has 2^26 samples (one 8192 x 8192 frame) or more; DESIGN.md s30 --, else
 * the cross-check.  Every route gives the same bits.  dwt_hip_window_route returns the route (0 or 2) a call with these
 * arguments takes under the calling thread's option, -1 for arguments dwt_hip_window_regions refuses or a batch below 1.
 * Ordered on the context's stream; no synchronisation, no copy between host and device, nothing allocated after the
 * first call of a shape; no result depends on what the scratch held (dwt_hip_fill_workspace).  A batch beyond
 * DWT_HIP_WINDOW_GRID_BATCH frames is covered by a loop inside the kernels.
 * Errors (nonzero, dwt_hip_last_error, nothing launched, nothing written): an unsupported wavelet, what
 * dwt_hip_window_regions refuses, a batch outside 1 .. 65535, null or host pointers, addresses or strides that are not
 * multiples of the element size, rows or frames that run into each other, a destination that shares a byte with any
 * source frame. */
#define DWT_HIP_WINDOW_TILE 64
#define DWT_HIP_WINDOW_GRID_BATCH 4096
int dwt_hip_window_regions(int wavelet, int size_x, int size_y, int j_max, int discard, int x0, int y0, int w, int h, int *xywh);
int dwt_hip_inverse_window_batch(int wavelet, const void *src, size_t batch_stride, int batch, int stride_x, int size_x, int size_y,
	int j_max, int discard, int x0, int y0, int w, int h, void *dst, size_t dst_batch_stride, int dst_stride_x);
int dwt_hip_window_route(int wavelet, int batch, int size_x, int size_y, int j_max, int discard, int x0, int y0, int w, int h);

/* dwt_util_perf_cdf97_2_s's protocol (src/libdwt.c:21444-21476) with the M images
 * resident in HBM: seconds per transform, minimum over N loops. */
void dwt_hip_perf_cdf97_2_s(int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int j_max, int decompose_one, int zero_padding,
	int M, int N, int clock_type, float *fwd_secs, float *inv_secs);

/* Kernel timing with HIP events on the stream the kernels run on.  While enabled,
 * every launch of the level-0 sweep kernel (the dominant kernel) is bracketed by
 * an event pair; dwt_hip_prof_read synchronises and returns the summed duration
 * and the number of launches since the last reset. */
void dwt_hip_prof_enable(int on); /* 1: level-0 kernel only; 2: every level's kernel */
int dwt_hip_prof_read(double *level0_ms_sum, int *launches);
/* mode 2: per-level sums (index = level whose input/output is the larger frame) */
int dwt_hip_prof_read_levels(double *ms_sum, int *launches, int n);

#ifdef __cplusplus
}
#endif
#endif
