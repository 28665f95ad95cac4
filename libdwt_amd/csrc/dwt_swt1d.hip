// dwt_swt1d.hip -- the stationary (undecimated) wavelet transform of a batch of rows, every level in ONE launch (gfx950).
//
// The reference (swt_cdf97_f_ex_stride_s / swt_cdf53_f_ex_stride_s, src/swt.c, over dwt_util_convolve1_s, src/util.c:5-48,
// and the saturating accessors of src/signal.c:43-93) filters a level's input x of N samples twice, with the low-pass
// and the high-pass filter g of 2c+1 taps dilated by u = 1 << level:
//
//     y = 0.0f;  for k = -c .. +c:  y = y + x[clamp(p - u*k, 0, N-1)] * g[k + c];   out[p] = y
//
// float32, product and sum rounded separately, from +0.0f, taps from the right neighbour to the left one, borders
// replicated (the reference's rule, SwtClamp) or, an extension, extended symmetrically (SwtReflect: the rule under which
// the transform has an inverse, dwt_iswt1d.hip; the border rule is a template parameter of the coefficient kernels).  Level l+1 filters the low-pass plane of level l.  Every plane has N samples: J levels turn N samples into
// 2*J*N coefficients.
//
// k_swt_lines: a line of up to N1D_MAX samples is loaded into LDS once; two LDS buffers hold the L chain, ping-ponged.
// NT threads work on a line (64: four lines per workgroup; 256: one), thread t takes samples t, t + NT, ... -- lanes read
// consecutive LDS addresses at every dilation -- and reads the 2*CL+1 taps once for both filters (the high-pass taps are
// a subset).  Coefficient mode stores H (and L where asked) with coalesced 4-byte stores.  Feature mode stores no
// coefficient: each level's plane is reduced as it is computed into the raw records of dwt_features.hip, with its
// accumulators and its order (thread t takes samples t, t + NT, ... there too, lanes by a shuffle tree, waves in index
// order), so the records are bit for bit those of k_feat_lines over the stored plane.  The passes that need the plane
// again -- the central moments about the mean, the four rounds of the median's radix select -- compute it again from
// the level's input, which is still in LDS.
//
// k_swt_level: one level through global memory, one thread per output sample, any byte strides: lines beyond N1D_MAX,
// strided elements, and the cross-check of the fused kernel (option "swt_fused" = 0).
#include "dwt_device.h"
#include "dwt_kernels.h"
#include "dwt_line_lds.h"

namespace dwt {

namespace {

#include "dwt_feat_acc.h"

#include "dwt_swt_taps.h"

template <class F, class B, bool FEAT, int NT, int CAP>
__global__ __launch_bounds__(256) void k_swt_lines(SwtLineArgs a)
{
	constexpr int LPW = 256 / NT;
	__shared__ float buf[LPW][2][CAP];
	__shared__ double shd[4];
	__shared__ u64 shk[4];
	__shared__ unsigned hist[FEAT ? LPW : 1][256];
	__shared__ unsigned sel[LPW][2];
	const int sub = threadIdx.x / NT, t = threadIdx.x % NT, N = a.N;
	const long line_raw = (long)blockIdx.x * LPW + sub;
	// (a workgroup's spare lines follow the last line through every barrier and write nothing)
	const bool active = line_raw < a.n_lines;
	const long line = active ? line_raw : a.n_lines - 1;
	const char *s = a.src + line * a.line_stride;
	float *cur = buf[sub][0], *nxt = buf[sub][1];

	line_to_lds(cur, s, N, 4, t, NT, a.vec);

	for (int l = 0; l < a.levels; l++) {
		__syncthreads();
		const int u = 1 << (a.level0 + l);
		const float *const in = cur;
		auto x = [&](int i) { return in[i]; };
		if constexpr (!FEAT) {
			float *const h_out = (float *)(a.dst_h + (long)l * a.plane_stride + line * a.dst_line_stride);
			float *const l_out = a.l_mode == 2                       ? (float *)(a.dst_l + (long)l * a.plane_stride + line * a.dst_line_stride)
			                     : a.l_mode == 1 && l == a.levels - 1 ? (float *)(a.dst_l + line * a.dst_line_stride)
			                                                          : nullptr;
			for (int p = t; p < N; p += NT) {
				float lo, hi;
				swt_point<F, int, B>(x, p, u, N, &lo, &hi);
				nxt[p] = lo;
				if (active) {
					h_out[p] = hi;
					if (l_out)
						l_out[p] = lo;
				}
			}
		} else {
			// the plane this level is reduced over, sample by sample: L was just written to nxt by this same thread
			float *const out = nxt;
			const int band = a.band;
			auto val = [&](int p) {
				if (band)
					return out[p];
				float lo, hi;
				swt_point<F, int>(x, p, u, N, &lo, &hi);
				return hi;
			};
			auto first = [&](int p) {
				float lo, hi;
				swt_point<F, int>(x, p, u, N, &lo, &hi);
				out[p] = lo;
				return band ? lo : hi;
			};
			reduce_record<NT>(t, N, first, val, line * a.levels + l, a.rec, a.nrec, a.work, a.pmode, a.p, active, shd, shk, hist[sub], sel[sub]);
		}
		float *const q = cur;
		cur = nxt;
		nxt = q;
	}
}

template <class F, class B>
__global__ __launch_bounds__(256) void k_swt_level(SwtLevelArgs a)
{
	const long p = (long)blockIdx.x * 256 + threadIdx.x, N = a.N, u = 1l << a.level;
	if (p >= N)
		return;
	for (long y = blockIdx.y; y < a.n_lines; y += gridDim.y) {
		const char *s = a.src + y * a.src_ls;
		const long es = a.src_es;
		float lo, hi;
		swt_point<F, long, B>([&](long i) { return *(const float *)(s + i * es); }, p, u, N, &lo, &hi);
		if (a.out_l)
			*(float *)(a.out_l + y * a.l_ls + p * a.l_es) = lo;
		if (a.out_l2)
			*(float *)(a.out_l2 + y * a.l2_ls + p * a.l2_es) = lo;
		if (a.out_h)
			*(float *)(a.out_h + y * a.h_ls + p * a.h_es) = hi;
	}
}

template <class F, class B, bool FEAT>
hipError_t swt_lines_t(const SwtLineArgs &a, hipStream_t s)
{
	// threads per line and LDS capacity: as k_feat_lines splits (64 threads up to 1024 samples), which fixes the order
	// of the feature sums; 32 KiB of LDS per workgroup up to 4096 samples, 64 KiB up to N1D_MAX
	if (a.N <= 1024)
		k_swt_lines<F, B, FEAT, 64, 1024><<<(unsigned)((a.n_lines + 3l) / 4), 256, 0, s>>>(a);
	else if (a.N <= 4096)
		k_swt_lines<F, B, FEAT, 256, 4096><<<a.n_lines, 256, 0, s>>>(a);
	else
		k_swt_lines<F, B, FEAT, 256, N1D_MAX><<<a.n_lines, 256, 0, s>>>(a);
	return hipGetLastError();
}

} // namespace

hipError_t launch_swt_lines(Wavelet w, bool features, const SwtLineArgs &a, hipStream_t s)
{
	if (a.n_lines <= 0 || a.levels <= 0)
		return hipSuccess;
	if (a.N < 1 || a.N > N1D_MAX || a.level0 < 0 || a.level0 + a.levels > SWT_MAX_LEVELS)
		return hipErrorInvalidValue;
	if (a.border != kSwtReplicate && (a.border != kSwtSymmetric || features)) // (the feature planes are the reference's: replicated)
		return hipErrorInvalidValue;
	if (w == kCdf97S)
		return features ? swt_lines_t<Swt97, SwtClamp, true>(a, s)
		                : a.border ? swt_lines_t<Swt97, SwtReflect, false>(a, s) : swt_lines_t<Swt97, SwtClamp, false>(a, s);
	if (w == kCdf53S)
		return features ? swt_lines_t<Swt53, SwtClamp, true>(a, s)
		                : a.border ? swt_lines_t<Swt53, SwtReflect, false>(a, s) : swt_lines_t<Swt53, SwtClamp, false>(a, s);
	return hipErrorInvalidValue;
}

hipError_t launch_swt_level(Wavelet w, const SwtLevelArgs &a, hipStream_t s)
{
	if (a.n_lines <= 0 || a.N <= 0)
		return hipSuccess;
	if (a.level < 0 || a.level >= SWT_MAX_LEVELS || (a.border != kSwtReplicate && a.border != kSwtSymmetric))
		return hipErrorInvalidValue;
	const dim3 grid((unsigned)((a.N + 255l) / 256), (unsigned)(a.n_lines < 65535 ? a.n_lines : 65535)); // (past the cap: tests/test_hip_grid_limits.py)
	if (w == kCdf97S && a.border)
		k_swt_level<Swt97, SwtReflect><<<grid, 256, 0, s>>>(a);
	else if (w == kCdf97S)
		k_swt_level<Swt97, SwtClamp><<<grid, 256, 0, s>>>(a);
	else if (w == kCdf53S && a.border)
		k_swt_level<Swt53, SwtReflect><<<grid, 256, 0, s>>>(a);
	else if (w == kCdf53S)
		k_swt_level<Swt53, SwtClamp><<<grid, 256, 0, s>>>(a);
	else
		return hipErrorInvalidValue;
	return hipGetLastError();
}

} // namespace dwt
