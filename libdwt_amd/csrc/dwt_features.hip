// dwt_features.hip -- the kernels of the per-subband feature statistics (dwt_util_wps_s, _mean_s, _var_s, _med_s, ...:
// src/libdwt.c:23086-23786) -- reductions and a selection over the subbands of a transformed image.
//
// What the kernels leave is RAW: per (image, band) record the sums as doubles (sum x, sum x^2, sum |x|^p, and about the
// float mean sum d^2, sum d^3, sum d^4), max |x| with the first index that holds it, and the median.  The host finishes
// them in float as the reference writes it (dwt_backend_features.hip).  The contract:
//   * sums accumulate in double in an order fixed by the band geometry alone -- per thread in index order, lanes by a
//     shuffle tree, waves and slabs in index order; no floating-point atomics -- so that a call gives the same bits on
//     every run and for every number of workgroups;
//   * x - mean is the float subtraction of the float mean, x*x and d^2 are exact in double, d^3 = d^2*d and
//     d^4 = d^2*d^2 are rounded once; |x|^p other than p = 1, 2 is pow in double rounded to float (as the EAW weights);
//   * max / argmax compare one 64-bit key, |x| bits above the complemented index: the largest |x|, then the lowest index;
//   * the median is a 4 x 8-bit radix select over the order-preserving integer image of the float: integer histogram
//     atomics, which commute.  NaN inputs are not pinned (the reference's qsort comparator is no order there).
//     FeatImgArgs::abs_key orders |x| instead (the key ignores the sign bit): the median magnitude of a band that is
//     only read, for the universal threshold.
//
// Lines of up to N1D_MAX samples: k_feat_lines, one workgroup per line, the line in LDS, every band of every level and
// every statistic from ONE read of the line.  Images and longer lines: bands cut into slabs of about FEAT_SLAB elements;
// k_feat_pass1 / _pass2 / _hist walk the slabs of all bands of all images of a batch in one launch each, k_feat_fold
// adds a band's slab partials in index order, k_feat_pick narrows the select by one byte.
#include "dwt_device.h"
#include "dwt_kernels.h"

namespace dwt {

namespace {

#include "dwt_feat_acc.h"

// ---- lines in LDS ----------------------------------------------------------------------------------------------------
template <int NT, int CAP>
__global__ __launch_bounds__(NT) void k_feat_lines(FeatLineArgs a)
{
	__shared__ float line[CAP];
	__shared__ double shd[4];
	__shared__ u64 shk[4];
	__shared__ unsigned hist[256];
	__shared__ unsigned sel[2];
	const int t = threadIdx.x, N = a.N;
	const long li = blockIdx.x;
	const float *row = (const float *)(a.src + li * a.line_stride);
	for (int i = 4 * t; i < N; i += 4 * NT) {
		if (i + 3 < N) {
			const f4u v = *(const f4u *)(row + i);
			line[i] = v.x;
			line[i + 1] = v.y;
			line[i + 2] = v.z;
			line[i + 3] = v.w;
		} else {
			for (int e = i; e < N; e++)
				line[e] = row[e];
		}
	}
	__syncthreads();
	for (int k = 0; k < a.nb; k++) {
		const float *b = line + a.off[k];
		const int n = a.len[k];
		const long r = li * a.nb + k;
		auto x = [&](int i) { return b[i]; };
		reduce_record<NT>(t, n, x, x, r, a.rec, a.nrec, a.work, a.pmode, a.p, true, shd, shk, hist, sel);
	}
}

// ---- images: slabs ---------------------------------------------------------------------------------------------------
struct Slab {
	int b, k; // image, band
	const char *p; // first element
	int w, r0, r1, c0, cn; // band width; rows r0 .. r1 and cn columns from c0, band coordinates
};

static __device__ __forceinline__ Slab slab_of(const FeatImgArgs &a, long g)
{
	Slab s;
	s.b = (int)(g / a.slabs);
	const int si = (int)(g % a.slabs);
	int k = 0;
	while (k + 1 < a.nb && a.bands[k + 1].slab0 <= si)
		k++;
	const FeatBand bd = a.bands[k];
	const int ls = si - bd.slab0, cc = ls % bd.ncc, rc = ls / bd.ncc;
	s.k = k;
	s.w = bd.w;
	s.c0 = cc * bd.cw;
	s.cn = min(bd.cw, bd.w - s.c0);
	s.r0 = rc * bd.rh;
	s.r1 = min(bd.h, s.r0 + bd.rh);
	s.p = a.img + (long)s.b * a.bstride + (long)bd.y0 * a.pitch + 4l * (bd.x0 + s.c0);
	return s;
}

// f(x, index within the band) over the slab's elements: a thread takes groups of four columns, its rows top to bottom
// -- which thread takes which element, and in what order, follows from the slab's shape alone
template <class F>
static __device__ __forceinline__ void walk_slab(const Slab &s, long pitch, F f)
{
	const int q = (s.cn + 3) >> 2;
	int lg = 0;
	while (lg < 8 && (1 << lg) < q)
		lg++;
	const int tx = threadIdx.x & ((1 << lg) - 1), ty = threadIdx.x >> lg, TX = 1 << lg, TY = 256 >> lg;
	for (int r = s.r0 + ty; r < s.r1; r += TY) {
		const float *row = (const float *)(s.p + (long)r * pitch);
		const unsigned i0 = (unsigned)r * (unsigned)s.w + (unsigned)s.c0;
		for (int g = tx; g < q; g += TX) {
			const int c = 4 * g;
			if (c + 3 < s.cn) {
				const f4u v = *(const f4u *)(row + c);
				f(v.x, i0 + c);
				f(v.y, i0 + c + 1);
				f(v.z, i0 + c + 2);
				f(v.w, i0 + c + 3);
			} else {
				for (int e = c; e < s.cn; e++)
					f(row[e], i0 + e);
			}
		}
	}
}

__global__ __launch_bounds__(256) void k_feat_pass1(FeatImgArgs a)
{
	__shared__ double shd[4];
	__shared__ u64 shk[4];
	const long total = (long)a.batch * a.slabs, np = total;
	for (long g = blockIdx.x; g < total; g += gridDim.x) {
		const Slab s = slab_of(a, g);
		Acc1 acc;
		walk_slab(s, a.pitch, [&](float x, unsigned idx) { acc.add(x, idx, a.pmode, a.p); });
		const double s1 = wg_sum<4>(acc.s1, shd), s2 = wg_sum<4>(acc.s2, shd);
		const double sp = a.pmode != kFeatPNone ? wg_sum<4>(acc.sp, shd) : 0.0;
		const u64 key = wg_max<4>(acc.key, shk);
		if (threadIdx.x == 0) {
			a.part[0 * np + g] = dbits(s1);
			a.part[1 * np + g] = dbits(s2);
			a.part[2 * np + g] = dbits(sp);
			a.part[3 * np + g] = key;
		}
	}
}

__global__ __launch_bounds__(256) void k_feat_pass2(FeatImgArgs a)
{
	__shared__ double shd[4];
	const long total = (long)a.batch * a.slabs, np = total;
	for (long g = blockIdx.x; g < total; g += gridDim.x) {
		const Slab s = slab_of(a, g);
		const FeatBand bd = a.bands[s.k];
		const float c = a.use_c ? a.c : mean_of(bitsd(a.rec[kFeatS1 * a.nrec + (long)s.b * a.nb + s.k]), (long)bd.w * bd.h);
		Acc2 m;
		walk_slab(s, a.pitch, [&](float x, unsigned) { m.add(x, c, a.mn); });
		const double m2 = wg_sum<4>(m.m2, shd), m3 = wg_sum<4>(m.m3, shd), m4 = wg_sum<4>(m.m4, shd);
		if (threadIdx.x == 0) {
			a.part[0 * np + g] = dbits(m2);
			a.part[1 * np + g] = dbits(m3);
			a.part[2 * np + g] = dbits(m4);
		}
	}
}

// one wave per (image, band): the band's slab partials, lane l those of slabs l, l + 64, ... in order, then the tree
__global__ __launch_bounds__(64) void k_feat_fold(FeatImgArgs a, int second)
{
	const int b = blockIdx.x / a.nb, k = blockIdx.x % a.nb, l = threadIdx.x;
	const FeatBand bd = a.bands[k];
	const long np = (long)a.batch * a.slabs, g0 = (long)b * a.slabs + bd.slab0, r = (long)b * a.nb + k;
	double v[3] = {0, 0, 0};
	u64 key = 0;
	for (int i = l; i < bd.nslab; i += 64) {
#pragma unroll
		for (int f = 0; f < 3; f++)
			v[f] += bitsd(a.part[f * np + g0 + i]);
		if (!second) {
			const u64 q = a.part[3 * np + g0 + i];
			key = q > key ? q : key;
		}
	}
#pragma unroll
	for (int f = 0; f < 3; f++)
		v[f] = wg_sum<1>(v[f], nullptr);
	key = wg_max<1>(key, nullptr);
	if (l == 0) {
		if (!second) {
			a.rec[kFeatS1 * a.nrec + r] = dbits(v[0]);
			a.rec[kFeatS2 * a.nrec + r] = dbits(v[1]);
			a.rec[kFeatSp * a.nrec + r] = dbits(v[2]);
			a.rec[kFeatKey * a.nrec + r] = key;
		} else {
			a.rec[kFeatM2 * a.nrec + r] = dbits(v[0]);
			a.rec[kFeatM3 * a.nrec + r] = dbits(v[1]);
			a.rec[kFeatM4 * a.nrec + r] = dbits(v[2]);
		}
	}
}

__global__ __launch_bounds__(256) void k_feat_hist(FeatImgArgs a, int pass)
{
	__shared__ unsigned hist[256];
	const long total = (long)a.batch * a.slabs;
	const int shift = 24 - 8 * pass;
	for (long g = blockIdx.x; g < total; g += gridDim.x) {
		const Slab s = slab_of(a, g);
		const long r = (long)s.b * a.nb + s.k;
		const unsigned prefix = pass ? a.sel[2 * r] : 0;
		hist[threadIdx.x] = 0;
		__syncthreads();
		walk_slab(s, a.pitch, [&](float x, unsigned) {
			const unsigned q = okey(a.abs_key ? fabsf(x) : x);
			if (pass == 0 || (q >> (shift + 8)) == prefix)
				atomicAdd(&hist[(q >> shift) & 255], 1u);
		});
		__syncthreads();
		const unsigned n = hist[threadIdx.x];
		if (n)
			atomicAdd(&a.hist[((long)pass * a.nrec + r) * 256 + threadIdx.x], n);
		__syncthreads();
	}
}

__global__ __launch_bounds__(64) void k_feat_pick(FeatImgArgs a, int pass)
{
	const long r = blockIdx.x;
	const FeatBand bd = a.bands[blockIdx.x % a.nb];
	unsigned prefix = pass ? a.sel[2 * r] : 0;
	unsigned rank = pass ? a.sel[2 * r + 1] : (unsigned)(((long)bd.w * bd.h) / 2);
	const unsigned bin = pick_bin(a.hist + ((long)pass * a.nrec + r) * 256, &rank);
	prefix = (prefix << 8) | bin;
	if (threadIdx.x == 0) {
		a.sel[2 * r] = prefix;
		a.sel[2 * r + 1] = rank;
		if (pass == 3)
			a.rec[kFeatMed * a.nrec + r] = to_bits(okey_inv(prefix));
	}
}

__global__ __launch_bounds__(256) void k_feat_abs(char *p, long sx, long sy, int w, int h)
{
	const int x = blockIdx.x * 256 + threadIdx.x;
	if (x >= w)
		return;
	for (int y = blockIdx.y; y < h; y += gridDim.y) {
		unsigned *e = (unsigned *)(p + (long)y * sx + (long)x * sy);
		*e &= 0x7fffffffu; // fabsf: the sign bit alone, NaN payloads kept
	}
}

} // namespace

hipError_t launch_feat_lines(const FeatLineArgs &a, hipStream_t s)
{
	if (a.n_lines <= 0 || a.nb <= 0)
		return hipSuccess;
	if (a.N > N1D_MAX || a.nb > 32)
		return hipErrorInvalidValue;
	if (a.N <= 1024)
		k_feat_lines<64, 1024><<<a.n_lines, 64, 0, s>>>(a);
	else
		k_feat_lines<256, N1D_MAX><<<a.n_lines, 256, 0, s>>>(a);
	return hipGetLastError();
}

static int slab_groups(const FeatImgArgs &a)
{
	const long total = (long)a.batch * a.slabs;
	const long want = a.groups > 0 ? a.groups : 256 * 8; // 8 workgroups on each of the 256 CUs
	return (int)(total < want ? total : want);
}

hipError_t launch_feat_pass1(const FeatImgArgs &a, hipStream_t s)
{
	k_feat_pass1<<<slab_groups(a), 256, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_feat_pass2(const FeatImgArgs &a, hipStream_t s)
{
	k_feat_pass2<<<slab_groups(a), 256, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_feat_fold(const FeatImgArgs &a, int second, hipStream_t s)
{
	k_feat_fold<<<a.batch * a.nb, 64, 0, s>>>(a, second);
	return hipGetLastError();
}

hipError_t launch_feat_hist(const FeatImgArgs &a, int pass, hipStream_t s)
{
	k_feat_hist<<<slab_groups(a), 256, 0, s>>>(a, pass);
	return hipGetLastError();
}

hipError_t launch_feat_pick(const FeatImgArgs &a, int pass, hipStream_t s)
{
	k_feat_pick<<<a.batch * a.nb, 64, 0, s>>>(a, pass);
	return hipGetLastError();
}

hipError_t launch_feat_abs(void *p, long sx, long sy, int w, int h, hipStream_t s)
{
	if (w <= 0 || h <= 0)
		return hipSuccess;
	dim3 grid((w + 255) / 256, h < 16384 ? h : 16384); // (past the cap: tests/test_hip_grid_limits.py)
	k_feat_abs<<<grid, 256, 0, s>>>((char *)p, sx, sy, w, h);
	return hipGetLastError();
}

} // namespace dwt
