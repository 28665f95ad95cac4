/*
 * libdwt.h -- drop-in declarations for the hot-path subset of libdwt's C API, served
 * by the MI355X backend (libdwt_amd/libdwt_hip.so).
 *
 * Written fresh: only the prototypes (names, argument order and meaning, in/out
 * conventions, error behaviour) follow the reference so that a program written
 * against xbarin02/libdwt -- e.g. its examples/simple/simple.c and
 * examples/simple-int/simple.c -- compiles and links unchanged.  Each block cites
 * the reference declaration it replaces (paths relative to the reference tree).
 *
 * Image addressing everywhere: element (y,x) lives at
 *     (char *)ptr + y*stride_x + x*stride_y
 * i.e. stride_x is the ROW pitch and stride_y the ELEMENT pitch, both in bytes
 * (src/inline.h:180-189).  "size_o_big" is the outer allocated frame, "size_i_big"
 * the inner image nested at its origin.
 *
 * `ptr` may be host memory (any strides; staged through HBM) or device memory
 * (see libdwt_hip.h).  Failures are logged and abort(), as dwt_util_error does in
 * the reference (src/libdwt.c:20410-20421); nothing falls back to a CPU path.
 */
#ifndef LIBDWT_H
#define LIBDWT_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- 2-D multi-level transforms, Mallat layout ---------------------------------- */

/* Forward float CDF 9/7, in place.  *j_max_ptr: requested levels in, levels done out;
 * negative or too large means "as many as possible".  src/libdwt.h:562-573. */
void dwt_cdf97_2f_s(void *ptr, int stride_x, int stride_y,
	int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int *j_max_ptr, int decompose_one, int zero_padding);

/* Inverse float CDF 9/7, in place.  j_max < 0 undoes a full decomposition.
 * src/libdwt.h:867-878. */
void dwt_cdf97_2i_s(void *ptr, int stride_x, int stride_y,
	int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int j_max, int decompose_one, int zero_padding);

/* Out-of-place variants: first level reads src, everything lands in dst.
 * src/libdwt.h:667-679, 962-974. */
void dwt_cdf97_2f_s2(const void *src, void *dst, int stride_x, int stride_y,
	int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int *j_max_ptr, int decompose_one, int zero_padding);
void dwt_cdf97_2i_s2(const void *src, void *dst, int stride_x, int stride_y,
	int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int j_max, int decompose_one, int zero_padding);

/* Reversible int32 CDF 5/3.  src/libdwt.h:686, 981. */
void dwt_cdf53_2f_i(void *ptr, int stride_x, int stride_y,
	int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int *j_max_ptr, int decompose_one, int zero_padding);
void dwt_cdf53_2i_i(void *ptr, int stride_x, int stride_y,
	int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int j_max, int decompose_one, int zero_padding);

/* EXTENSION: reversible int16 CDF 5/3 in JPEG 2000 order (ITU-T T.800 F.3.8.1 reversible 1-D filtering, F.3.2 2D_SD:
 * every level lifts its columns, then its rows; the inverse the rows, then the columns).  The reference has this
 * transform only as a single-level core (examples/cores/cores.c: cores2f_cdf53_v2x2_i16 / cores2i_cdf53_v2x2_i16); these
 * entries take the parameter list of dwt_cdf53_2f_i / dwt_cdf53_2i_i, int16_t samples (stride_y >= 2), the same Mallat
 * layout and j_max rules.  The inverse restores every int16 image bit for bit.  DESIGN.md s20. */
void dwt_cdf53_2f_i16(void *ptr, int stride_x, int stride_y,
	int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int *j_max_ptr, int decompose_one, int zero_padding);
void dwt_cdf53_2i_i16(void *ptr, int stride_x, int stride_y,
	int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int j_max, int decompose_one, int zero_padding);

/* EXTENSION: float CDF 9/7 on IEEE binary16 storage.  The parameter list, Mallat layout and j_max rules of dwt_cdf97_2f_s /
 * dwt_cdf97_2i_s; samples are binary16 bit patterns (stride_y >= 2).  Every level widens its frame to binary32 (exact),
 * computes what one level of dwt_cdf97_2f_s / _2i_s computes, and rounds the result to binary16 once, to nearest even.  Not
 * reversible (a 5-level round trip of 8-bit data returns within one grey level: 0.625 measured on 8192 x 8192) and not protected against overflow: a
 * level doubles the gain of the LL band, so max|x| * 2^levels must stay below 65504 (8-bit data: 8 levels; 12-bit data: 3),
 * beyond which coefficients become +-Inf and NaN as IEEE arithmetic has it.  DESIGN.md s22. */
void dwt_cdf97_2f_h(void *ptr, int stride_x, int stride_y,
	int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int *j_max_ptr, int decompose_one, int zero_padding);
void dwt_cdf97_2i_h(void *ptr, int stride_x, int stride_y,
	int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int j_max, int decompose_one, int zero_padding);

/* Float CDF 5/3.  src/libdwt.h:722, 1053. */
void dwt_cdf53_2f_s(void *ptr, int stride_x, int stride_y,
	int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int *j_max_ptr, int decompose_one, int zero_padding);
void dwt_cdf53_2i_s(void *ptr, int stride_x, int stride_y,
	int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int j_max, int decompose_one, int zero_padding);

/* Fixed-point int32 CDF 9/7.  src/libdwt.h:704, 999. */
void dwt_cdf97_2f_i(void *ptr, int stride_x, int stride_y,
	int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int *j_max_ptr, int decompose_one, int zero_padding);
void dwt_cdf97_2i_i(void *ptr, int stride_x, int stride_y,
	int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int j_max, int decompose_one, int zero_padding);

/* Double precision CDF 9/7 and 5/3 (elements of 8 bytes).  src/libdwt.h:526, 831, 544, 849. */
void dwt_cdf97_2f_d(void *ptr, int stride_x, int stride_y,
	int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int *j_max_ptr, int decompose_one, int zero_padding);
void dwt_cdf97_2i_d(void *ptr, int stride_x, int stride_y,
	int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int j_max, int decompose_one, int zero_padding);
void dwt_cdf53_2f_d(void *ptr, int stride_x, int stride_y,
	int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int *j_max_ptr, int decompose_one, int zero_padding);
void dwt_cdf53_2i_d(void *ptr, int stride_x, int stride_y,
	int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int j_max, int decompose_one, int zero_padding);

/* Interleaved (in-place lifting) layout: no de-interleave, level j works on the
 * stride-2^j lattice of the image.  src/libdwt.h:586, 889, 599, 944.  The 9/7 pair runs its
 * rows and columns in interleaved phases in the reference (src/libdwt.c:12970-13480,
 * 17517-17594), which rounds differently from rows-then-columns in the top 8 rows and the last
 * 5 columns of a level.  Bit-identical to the reference BY DEFAULT: the fused sweep's two border
 * strips are recomputed in the reference's phase order (k_il_strip); dwt_util_set_accel(1) runs
 * that order pass by pass over the whole image (the cross-check).  The 5/3 pair is bit-identical
 * either way. */
void dwt_cdf97_2f_inplace_s(void *ptr, int stride_x, int stride_y,
	int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int *j_max_ptr, int decompose_one, int zero_padding);
void dwt_cdf97_2i_inplace_s(void *ptr, int stride_x, int stride_y,
	int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int j_max, int decompose_one, int zero_padding);
void dwt_cdf53_2f_inplace_s(void *ptr, int stride_x, int stride_y,
	int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int *j_max_ptr, int decompose_one, int zero_padding);
void dwt_cdf53_2i_inplace_s(void *ptr, int stride_x, int stride_y,
	int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int j_max, int decompose_one, int zero_padding);
/* level count only, no transform (src/libdwt.h:779, src/libdwt.c:16780) */
void dwt_cdf53_2f_dummy_s(void *ptr, int stride_x, int stride_y,
	int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int *j_max_ptr, int decompose_one);
/* fixed-point int32 CDF 9/7, interleaved in place (src/libdwt.h:1035, 1017).  As in the reference
 * the strides are not scaled per level: above one level the dense top-left block is transformed
 * again (src/libdwt.c:17423 "tested only with j=1"); bit-identical, forward + inverse restore
 * the image exactly for any level count. */
void dwt_cdf97_2f_inplace_i(void *ptr, int stride_x, int stride_y,
	int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int *j_max_ptr, int decompose_one, int zero_padding);
void dwt_cdf97_2i_inplace_i(void *ptr, int stride_x, int stride_y,
	int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int j_max, int decompose_one, int zero_padding);
/* the reference's other CPU schedules of the same forward transform (identical bits):
 * src/libdwt.h:612, 625, 649 */
void dwt_cdf97_2f_inplace_sep_s(void *ptr, int stride_x, int stride_y,
	int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int *j_max_ptr, int decompose_one, int zero_padding);
void dwt_cdf97_2f_inplace_sep_sdl_s(void *ptr, int stride_x, int stride_y,
	int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int *j_max_ptr, int decompose_one, int zero_padding);
void dwt_cdf97_2f_inplace_sdl_s(void *ptr, int stride_x, int stride_y,
	int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int *j_max_ptr, int decompose_one, int zero_padding);

/* ---- 1-D multi-level transforms, float, Mallat layout (L_J, then H_J .. H_1) --------- */

/* Forward CDF 9/7 / 5/3 of one line, in place; elements stride_y bytes apart.  *j_max_ptr:
 * requested levels in, levels done out (negative or above ceil(log2(size_o_big_x)): all).
 * src/libdwt.h:1128, 1144. */
void dwt_cdf97_1f_s(void *ptr, int stride_y, int size_o_big_x, int size_i_big_x, int *j_max_ptr, int zero_padding);
void dwt_cdf53_1f_s(void *ptr, int stride_y, int size_o_big_x, int size_i_big_x, int *j_max_ptr, int zero_padding);

/* Inverse of the above; j_max < 0 (or too large) undoes a full decomposition.  src/libdwt.h:1185, 1201. */
void dwt_cdf97_1i_s(void *ptr, int stride_y, int size_o_big_x, int size_i_big_x, int j_max, int zero_padding);
void dwt_cdf53_1i_s(void *ptr, int stride_y, int size_o_big_x, int size_i_big_x, int j_max, int zero_padding);

/* Forward 1-D transform of each of the rows 0 .. size_i_big_y-1 ("series"), rows stride_x bytes
 * apart; size_o_big_y is not used.  One batched call.  src/libdwt.h:1233, 1252. */
void dwt_cdf97_2f1_s(void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int *j_max_ptr, int zero_padding);
void dwt_cdf53_2f1_s(void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int *j_max_ptr, int zero_padding);

/* ---- interpolating 5/3 wavelet, float --------------------------------------------------- */

/* CDF 5/3 with the predict step only (no update), then the CDF 5/3 scaling; Mallat layout, in place, all
 * arguments as for dwt_cdf53_2f_s / _2i_s and dwt_cdf53_1f_s / _1i_s.  src/libdwt.h:813, 1108, 1160, 1217;
 * src/libdwt.c:16801, 18457, 16166, 15900. */
void dwt_interp53_2f_s(void *ptr, int stride_x, int stride_y,
	int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int *j_max_ptr, int decompose_one, int zero_padding);
void dwt_interp53_2i_s(void *ptr, int stride_x, int stride_y,
	int size_o_big_x, int size_o_big_y, int size_i_big_x, int size_i_big_y,
	int j_max, int decompose_one, int zero_padding);
void dwt_interp53_1f_s(void *ptr, int stride_y, int size_o_big_x, int size_i_big_x, int *j_max_ptr, int zero_padding);
void dwt_interp53_1i_s(void *ptr, int stride_y, int size_o_big_x, int size_i_big_x, int j_max, int zero_padding);

/* ---- edge-avoiding CDF 5/3 wavelets (EAW, Fattal 2009), float -------------------------- */

/* Forward, Mallat layout, in place.  Allocates wH[j] (size_o_src_y x size_i_src_x, row-major) and wV[j]
 * (size_o_src_x x size_i_src_y, column-major) of every level j with dwt_util_alloc -- host memory the caller
 * free()s -- and fills them; so a call on device memory copies its weights to the host (8 bytes per sample of
 * each level).  Entries of one-sample lines are not written (the reference leaves them uninitialised).
 * alpha 1 and 0 are bit-exact; any other alpha is within 1 ulp in the weights (include/libdwt_hip.h).
 * src/libdwt.h:742, src/libdwt.c:16663. */
void dwt_eaw53_2f_s(void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int *j_max_ptr, int decompose_one, int zero_padding,
	float *wH[], float *wV[], float alpha);

/* Inverse of the above with the forward's weights (host arrays).  src/libdwt.h:1073, src/libdwt.c:18373. */
void dwt_eaw53_2i_s(void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int j_max, int decompose_one, int zero_padding,
	float *wH[], float *wV[]);

/* Interleaved layout (level j on the lattice of stride 2^j over the inner frame); wH[j], wV[j] both
 * size_i_src_y x size_i_src_x (wV column-major); zero_padding is not used.  src/libdwt.h:758, 1088;
 * src/libdwt.c:16602, 17932. */
void dwt_eaw53_2f_inplace_s(void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int *j_max_ptr, int decompose_one, int zero_padding,
	float *wH[], float *wV[], float alpha);
void dwt_eaw53_2i_inplace_s(void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int j_max, int decompose_one, int zero_padding,
	float *wH[], float *wV[]);

/* Only clamps *j_max_ptr as the forward would.  src/libdwt.h:796, src/libdwt.c:16759. */
void dwt_eaw53_2f_dummy_s(void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int *j_max_ptr, int decompose_one);

/* malloc(elems * elem_size): what the EAW forward allocates its weights with.  src/libdwt.h:3743. */
void *dwt_util_alloc(int elems, size_t elem_size);

/* ---- lifecycle and backend knobs (src/libdwt.h:1667-1745, 1974-1986) -------------- */
void dwt_util_init(void);   /* brings the device up (the reference loads BCE firmware here) */
void dwt_util_finish(void); /* releases device workspace */
void dwt_util_abort(void);

/* Acceleration selector.  The reference's values 0..16 choose among CPU loop
 * schedules that all give the same coefficients (src/libdwt.h:1703-1720); here 0
 * (default) runs the fused tile-sweep kernels and 1 the exact line-pass kernels;
 * any other value is accepted and treated as 0. */
void dwt_util_set_accel(int accel_type);
int dwt_util_get_accel(void);
/* Accepted for source compatibility; the device schedules its own waves. */
void dwt_util_set_num_threads(int num_threads);
int dwt_util_get_num_threads(void);
int dwt_util_get_max_threads(void);
void dwt_util_set_num_workers(int num_workers);
int dwt_util_get_num_workers(void);

/* ---- image helpers used by the examples (host memory) ---------------------------- */
/* src/libdwt.h:2231, 2242 (next prime >= min_stride on x86_64; eight layouts) */
int dwt_util_get_opt_stride(int min_stride);
int dwt_util_get_stride(int min_stride, int opt);
/* src/libdwt.h:2847 */
size_t dwt_util_image_size(int stride_x, int stride_y, int size_o_big_x, int size_o_big_y);
/* src/libdwt.c:1437, 1482 */
void dwt_util_alloc_image(void **pptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y);
void dwt_util_free_image(void **pptr);
/* synthetic test patterns, src/libdwt.c:1338, 1270 */
void dwt_util_test_image_fill_s(void *ptr, int stride_x, int stride_y, int size_i_big_x, int size_i_big_y, int rand);
void dwt_util_test_image_fill_i(void *ptr, int stride_x, int stride_y, int size_i_big_x, int size_i_big_y, int rand);
/* the other synthetic patterns, selected by `type` (src/libdwt.h:1438, 1421; src/libdwt.c:1201-1244) */
void dwt_util_test_image_fill2_s(void *ptr, int stride_x, int stride_y, int size_i_big_x, int size_i_big_y, int rand, int type);
void dwt_util_test_image_fill2_i(void *ptr, int stride_x, int stride_y, int size_i_big_x, int size_i_big_y, int rand, int type);
/* the int patterns (types 0 and 2) in int16_t samples, src/libdwt.h:1325 */
void dwt_util_test_image_fill2_i16(void *ptr, int stride_x, int stride_y, int size_i_big_x, int size_i_big_y, int rand, int type);
/* src/libdwt.c:21154, 21235 */
void dwt_util_copy_s(const void *src, void *dst, int stride_x, int stride_y, int size_i_big_x, int size_i_big_y);
void dwt_util_copy_i(const void *src, void *dst, int stride_x, int stride_y, int size_i_big_x, int size_i_big_y);
/* returns 0 when equal: float within 1e-3 absolute and finite, int exactly
 * (src/libdwt.c:1593-1620, 1531-1558) */
int dwt_util_compare_s(void *ptr1, void *ptr2, int stride_x, int stride_y, int size_i_big_x, int size_i_big_y);
int dwt_util_compare_i(void *ptr1, void *ptr2, int stride_x, int stride_y, int size_i_big_x, int size_i_big_y);
/* log-magnitude view of a transform, src/libdwt.c:21075, 21020 */
void dwt_util_conv_show_s(const void *src, void *dst, int stride_x, int stride_y, int size_i_big_x, int size_i_big_y);
void dwt_util_conv_show_i(const void *src, void *dst, int stride_x, int stride_y, int size_i_big_x, int size_i_big_y);
/* |x| of int16_t samples, stored as int16_t, src/libdwt.h:2460 */
void dwt_util_conv_show_i16(const void *src, void *dst, int stride_x, int stride_y, int size_i_big_x, int size_i_big_y);
/* EXTENSION: host images of float samples <-> IEEE binary16 samples, element (y, x) of either at y * stride_x + x * stride_y
 * bytes.  float -> half rounds to nearest even (|x| >= 65520 to Inf, results below 2^-14 subnormal, NaN to a quiet NaN);
 * half -> float is exact. */
void dwt_util_float_to_half(void *dst, int dst_stride_x, int dst_stride_y, const void *src, int src_stride_x, int src_stride_y,
	int size_x, int size_y);
void dwt_util_half_to_float(void *dst, int dst_stride_x, int dst_stride_y, const void *src, int src_stride_x, int src_stride_y,
	int size_x, int size_y);
/* double-precision twins (examples/simple-double): pattern with 0-based x, y
 * (src/libdwt.c:1112-1125), copy, compare within 1e-6 absolute, view, PGM writer */
void dwt_util_test_image_fill_d(void *ptr, int stride_x, int stride_y, int size_i_big_x, int size_i_big_y, int rand);
void dwt_util_copy_d(const void *src, void *dst, int stride_x, int stride_y, int size_i_big_x, int size_i_big_y);
int dwt_util_compare_d(void *ptr1, void *ptr2, int stride_x, int stride_y, int size_i_big_x, int size_i_big_y);
void dwt_util_conv_show_d(const void *src, void *dst, int stride_x, int stride_y, int size_i_big_x, int size_i_big_y);
int dwt_util_save_to_pgm_d(const char *filename, double max_value, const void *ptr, int stride_x, int stride_y,
	int size_i_big_x, int size_i_big_y);
/* ASCII PGM writers, src/libdwt.h:1755, 1783; return 0 on success */
int dwt_util_save_to_pgm_s(const char *filename, float max_value, const void *ptr, int stride_x, int stride_y,
	int size_i_big_x, int size_i_big_y);
int dwt_util_save_to_pgm_i(const char *filename, int max_value, const void *ptr, int stride_x, int stride_y,
	int size_i_big_x, int size_i_big_y);
/* int16_t samples, src/libdwt.h:1765 */
int dwt_util_save_to_pgm_i16(const char *filename, int16_t max_value, const void *ptr, int stride_x, int stride_y,
	int size_i_big_x, int size_i_big_y);
/* src/libdwt.h:1799 (src/libdwt.c:19727-19792): log(1 + |x|) of every sample (dwt_util_conv_show_s), scaled
 * to the largest of them, as an ASCII PGM; returns 0 */
int dwt_util_save_log_to_pgm_s(const char *path, const void *ptr, int stride_x, int stride_y, int size_x, int size_y);
/* ASCII PGM readers: allocate the image with the optimal stride (src/libdwt.h:1894, 1926);
 * 0 on success, 1 open, 2 header, 3 depth, 4 data, 5 sample out of range */
int dwt_util_load_from_pgm_s(const char *filename, float max_value, void **pptr, int *pstride_x, int *pstride_y,
	int *psize_x, int *psize_y);
int dwt_util_load_from_pgm_i(const char *filename, int max_value, void **pptr, int *pstride_x, int *pstride_y,
	int *psize_x, int *psize_y);
/* int16_t samples (stride_y 2), src/libdwt.h:1936 */
int dwt_util_load_from_pgm_i16(const char *filename, int16_t max_value, void **pptr, int *pstride_x, int *pstride_y,
	int *psize_x, int *psize_y);
/* text matrices ("MAT": one row per line, comma separated), src/libdwt.h:1829, 1909, 1951 */
int dwt_util_save_to_mat_s(const char *path, const void *ptr, int size_x, int size_y, int stride_x, int stride_y);
int dwt_util_load_from_mat_s(const char *path, void **ptr, int *size_x, int *size_y, int *stride_x, int *stride_y);
int dwt_util_load_from_mat_i(const char *path, void **ptr, int *size_x, int *size_y, int *stride_x, int *stride_y);

/* ---- subband addressing (src/libdwt.h:2276-2330, src/libdwt.c:20731-20950) -------- */
enum dwt_subbands { DWT_LL, DWT_HL, DWT_LH, DWT_HH };
/* Address and size of a subband after j_max levels.  Pure address arithmetic: valid
 * for host and for device images. */
void dwt_util_subband(void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int j_max, enum dwt_subbands band,
	void **dst_ptr, int *dst_size_x, int *dst_size_y);
void dwt_util_subband_s(void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int j_max, enum dwt_subbands band,
	void **dst_ptr, int *dst_size_x, int *dst_size_y);
void dwt_util_subband_i(void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int j_max, enum dwt_subbands band,
	void **dst_ptr, int *dst_size_x, int *dst_size_y);

/* Feature vectors of a transformed image (src/libdwt.h:2875-3309): one float per non-empty detail band of levels
 * 1 .. j_max-1 (level j_max itself is not visited), HL, LH, HH within a level; dwt_util_count_subbands_s of them.
 * ptr is host or device memory, fv host memory.  The bands are reduced on the device: sums in double in a fixed
 * order, rounded once and finished in float; maxnorm, maxidx and med are exact for NaN-free input (med as a value;
 * NaN inputs are not pinned).  See include/libdwt_hip.h. */
int dwt_util_count_subbands_s(const void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int j_max);
void dwt_util_wps_s(const void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int j_max, float *fv);
void dwt_util_maxidx_s(const void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int j_max, float *fv);
void dwt_util_mean_s(const void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int j_max, float *fv);
void dwt_util_med_s(const void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int j_max, float *fv);
void dwt_util_var_s(const void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int j_max, float *fv);
void dwt_util_stdev_s(const void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int j_max, float *fv);
void dwt_util_skew_s(const void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int j_max, float *fv);
void dwt_util_kurt_s(const void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int j_max, float *fv);
void dwt_util_maxnorm_s(const void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int j_max, float *fv);
void dwt_util_norm_s(const void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int j_max, float *fv);
void dwt_util_lpnorm_s(const void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int j_max, float *fv, float p);
/* one statistic of one band of size_x x size_y coefficients */
float dwt_util_band_wps_s(const void *ptr, int stride_x, int stride_y, int size_x, int size_y, int j);
float dwt_util_band_maxidx_s(const void *ptr, int stride_x, int stride_y, int size_x, int size_y);
float dwt_util_band_mean_s(const void *ptr, int stride_x, int stride_y, int size_x, int size_y);
float dwt_util_band_med_s(const void *ptr, int stride_x, int stride_y, int size_x, int size_y);
float dwt_util_band_var_s(const void *ptr, int stride_x, int stride_y, int size_x, int size_y);
float dwt_util_band_stdev_s(const void *ptr, int stride_x, int stride_y, int size_x, int size_y);
float dwt_util_band_skew_s(const void *ptr, int stride_x, int stride_y, int size_x, int size_y);
float dwt_util_band_kurt_s(const void *ptr, int stride_x, int stride_y, int size_x, int size_y);
float dwt_util_band_maxnorm_s(const void *ptr, int stride_x, int stride_y, int size_x, int size_y);
float dwt_util_band_norm_s(const void *ptr, int stride_x, int stride_y, int size_x, int size_y);
float dwt_util_band_lpnorm_s(const void *ptr, int stride_x, int stride_y, int size_x, int size_y, float p);
float dwt_util_band_moment_s(const void *ptr, int stride_x, int stride_y, int size_x, int size_y, int n, float c);
float dwt_util_band_cmoment_s(const void *ptr, int stride_x, int stride_y, int size_x, int size_y, int n);
float dwt_util_band_smoment_s(const void *ptr, int stride_x, int stride_y, int size_x, int size_y, int n);
void dwt_util_subband_const_s(const void *ptr, int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int j_max, enum dwt_subbands band, const void **dst_ptr, int *dst_size_x, int *dst_size_y);
/* |x| in place, host or device memory */
void dwt_util_abs_s(void *ptr, int stride_x, int stride_y, int size_x, int size_y);
/* ---- conditioning of spectra (src/libdwt.h; src/libdwt.c:25426-26055): NOTE the sizes come before the strides.  Host
 * or device memory; DESIGN.md s16 states what is bit-identical to the reference and how the centre is decided --------- */
int dwt_util_find_min_max_s(const void *ptr, int size_x, int size_y, int stride_x, int stride_y, float *min, float *max);
int dwt_util_shift_s(void *ptr, int size_x, int size_y, int stride_x, int stride_y, float a);
int dwt_util_scale_s(void *ptr, int size_x, int size_y, int stride_x, int stride_y, float a);
/* every row's range mapped to [lo, hi]; constant rows are left alone (one summary warning) */
int dwt_util_scale21_s(void *ptr, int size_x, int size_y, int stride_x, int stride_y, float lo, float hi);
/* row[x] = row[x + displ_x], the border sample / zero moving in */
int dwt_util_displace1_s(void *ptr, int size_x, int stride_y, int displ_x);
int dwt_util_displace1_zero_s(void *ptr, int size_x, int stride_y, int displ_x);
int dwt_util_get_center1_s(const void *ptr, int size_x, int stride_y);
int dwt_util_center1_s(void *ptr, int size_x, int stride_y, int max_iters);
int dwt_util_center21_s(void *ptr, int size_x, int size_y, int stride_x, int stride_y, int max_iters);
/* every row minus its median */
void dwt_util_shift21_med_s(void *ptr, int size_x, int size_y, int stride_x, int stride_y);
/* pointer arithmetic only: the address of (offset_y, offset_x) / of the len_x columns about the centre column */
void *dwt_util_viewport(void *ptr, int size_x, int size_y, int stride_x, int stride_y, int offset_x, int offset_y);
void *dwt_util_crop21(void *ptr, int size_x, int size_y, int stride_x, int stride_y, int len_x);
float *dwt_util_addr_coeff_s(void *ptr, int y, int x, int stride_x, int stride_y); /* src/libdwt.c:1064 */
int *dwt_util_addr_coeff_i(void *ptr, int y, int x, int stride_x, int stride_y);

/* ---- measurement and self-test helpers (src/libdwt.h:2618-2760; src/libdwt.c:21262,
 * 21391, 22296, 22559, 23788, 23877, 24163, 24203) ---------------------------------- */
enum dwt_array { DWT_ARR_SIMPLE, DWT_ARR_SPARSE, DWT_ARR_PACKED };
int dwt_util_pow2_ceil_log2(int x);
void dwt_util_get_sizes_s(enum dwt_array array_type, int size_x, int size_y, int opt_stride,
	int *stride_x, int *stride_y, int *size_o_big_x, int *size_o_big_y, int *size_i_big_x, int *size_i_big_y);
void dwt_util_get_sizes_i(enum dwt_array array_type, int size_x, int size_y, int opt_stride,
	int *stride_x, int *stride_y, int *size_o_big_x, int *size_o_big_y, int *size_i_big_x, int *size_i_big_y);
/* M transforms per loop, minimum over N loops, seconds per transform; host images (the
 * call is timed as a drop-in user sees it, staging included) */
void dwt_util_perf_cdf97_2_s(int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int j_max, int decompose_one, int zero_padding,
	int M, int N, int clock_type, float *fwd_secs, float *inv_secs);
void dwt_util_perf_cdf53_2_i(int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int j_max, int decompose_one, int zero_padding,
	int M, int N, int clock_type, float *fwd_secs, float *inv_secs);
/* round-trip self-tests: 0 = success */
int dwt_util_test_cdf97_2_s(int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int j_max, int decompose_one, int zero_padding);
int dwt_util_test_cdf97_2_s2(int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int j_max, int decompose_one, int zero_padding);
int dwt_util_test2_cdf97_2_s(enum dwt_array array_type, int size_x, int size_y, int opt_stride, int j_max, int decompose_one);
int dwt_util_test2_cdf97_2_s2(enum dwt_array array_type, int size_x, int size_y, int opt_stride, int j_max, int decompose_one);
/* the same self-tests for the double and the fixed-point int 9/7 drivers (src/libdwt.h:2688,
 * 2703, 2727, 2739; examples/test/test.c:61-73) */
void dwt_util_get_sizes_d(enum dwt_array array_type, int size_x, int size_y, int opt_stride,
	int *stride_x, int *stride_y, int *size_o_big_x, int *size_o_big_y, int *size_i_big_x, int *size_i_big_y);
int dwt_util_test_cdf97_2_d(int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int j_max, int decompose_one, int zero_padding);
int dwt_util_test_cdf97_2_i(int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int j_max, int decompose_one, int zero_padding);
int dwt_util_test2_cdf97_2_d(enum dwt_array array_type, int size_x, int size_y, int opt_stride, int j_max, int decompose_one);
int dwt_util_test2_cdf97_2_i(enum dwt_array array_type, int size_x, int size_y, int opt_stride, int j_max, int decompose_one);

/* ---- timers (src/libdwt.h:1589-1658) --------------------------------------------- */
enum dwt_timer_types {
	DWT_TIME_CLOCK_GETTIME,
	DWT_TIME_CLOCK_GETTIME_REALTIME,
	DWT_TIME_CLOCK_GETTIME_MONOTONIC,
	DWT_TIME_CLOCK_GETTIME_MONOTONIC_RAW,
	DWT_TIME_CLOCK_GETTIME_PROCESS_CPUTIME_ID,
	DWT_TIME_CLOCK_GETTIME_THREAD_CPUTIME_ID,
	DWT_TIME_CLOCK,
	DWT_TIME_TIMES,
	DWT_TIME_GETRUSAGE,
	DWT_TIME_GETRUSAGE_SELF,
	DWT_TIME_GETRUSAGE_CHILDREN,
	DWT_TIME_GETRUSAGE_THREAD,
	DWT_TIME_GETTIMEOFDAY,
	DWT_TIME_IOCTL_RTC,
	DWT_TIME_AUTOSELECT
};
typedef int64_t dwt_clock_t;
int dwt_util_clock_available(int type);
int dwt_util_clock_autoselect(void);
dwt_clock_t dwt_util_get_frequency(int type);
dwt_clock_t dwt_util_get_clock(int type);

/* ---- logging and identification (src/libdwt.h:2154-2224, 1577-1582) --------------- */
enum dwt_util_loglevel { LOG_NONE = 0, LOG_DBG, LOG_INFO, LOG_WARN, LOG_ERR, LOG_TEST };
int dwt_util_log(enum dwt_util_loglevel level, const char *format, ...);
void dwt_util_error(const char *format, ...);
const char *dwt_util_version(void);
const char *dwt_util_arch(void);
const char *dwt_util_node(void);
const char *dwt_util_appname(void);

/* size sweep writing "pixels<TAB>seconds per pixel" rows (src/libdwt.c:22559) */
void dwt_util_measure_perf_cdf97_2_s(enum dwt_array array_type, int min_x, int max_x, int opt_stride,
	int j_max, int decompose_one, int zero_padding, int M, int N, int clock_type,
	FILE *fwd_plot_data, FILE *inv_plot_data);
/* the same protocols for the interleaved-layout entries (src/libdwt.h:2520, 2537, 2554, 2576,
 * 2744, 2764, 2784, 2804) */
void dwt_util_perf_cdf97_2_inplace_s(int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int j_max, int decompose_one, int zero_padding,
	int M, int N, int clock_type, float *fwd_secs, float *inv_secs);
void dwt_util_measure_perf_cdf97_2_inplace_s(enum dwt_array array_type, int min_x, int max_x, int opt_stride,
	int j_max, int decompose_one, int zero_padding, int M, int N, int clock_type,
	FILE *fwd_plot_data, FILE *inv_plot_data);
void dwt_util_perf_cdf97_2_inplace_sep_s(int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int j_max, int decompose_one, int zero_padding,
	int M, int N, int clock_type, float *fwd_secs, float *inv_secs);
void dwt_util_measure_perf_cdf97_2_inplace_sep_s(enum dwt_array array_type, int min_x, int max_x, int opt_stride,
	int j_max, int decompose_one, int zero_padding, int M, int N, int clock_type,
	FILE *fwd_plot_data, FILE *inv_plot_data);
void dwt_util_perf_cdf97_2_inplace_sep_sdl_s(int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int j_max, int decompose_one, int zero_padding,
	int M, int N, int clock_type, float *fwd_secs, float *inv_secs);
void dwt_util_measure_perf_cdf97_2_inplace_sep_sdl_s(enum dwt_array array_type, int min_x, int max_x, int opt_stride,
	int j_max, int decompose_one, int zero_padding, int M, int N, int clock_type,
	FILE *fwd_plot_data, FILE *inv_plot_data);
void dwt_util_perf_cdf97_2_inplace_sdl_s(int stride_x, int stride_y, int size_o_big_x, int size_o_big_y,
	int size_i_big_x, int size_i_big_y, int j_max, int decompose_one, int zero_padding,
	int M, int N, int clock_type, float *fwd_secs, float *inv_secs);
void dwt_util_measure_perf_cdf97_2_inplace_sdl_s(enum dwt_array array_type, int min_x, int max_x, int opt_stride,
	int j_max, int decompose_one, int zero_padding, int M, int N, int clock_type,
	FILE *fwd_plot_data, FILE *inv_plot_data);

#ifdef __cplusplus
}
#endif
#endif
