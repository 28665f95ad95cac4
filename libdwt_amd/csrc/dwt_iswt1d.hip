// dwt_iswt1d.hip -- the inverse stationary wavelet transform of a batch of rows under the symmetric border, every level in
// ONE launch (gfx950).  An extension: the reference stops at the forward functions.
//
// With u = 1 << level, the synthesis filters sl (2*CH+1 taps) and sh (2*CL+1 taps) of dwt_swt_taps.h and the level's planes
// L and H of N samples, for every p:
//
//     x[p] = 0.5f * (conv(L, sl, u)[p] + conv(H, sh, u)[p]),   conv(x, g, u)[p] = sum over k = -c .. +c of x[reflect(p - u*k)] * g[k + c]
//
// float32, every product and sum rounded on its own, each conv from +0.0f in the order of the forward's tap sum.  Levels run
// from levels-1 down to 0; level l's output is the L plane of level l-1.  A detail coefficient passes through its plane's
// band operator (KEEP, ZERO, SCALE, HARD, SOFT; dwt_band_op.h) as it is read; a ZERO plane is never read.
//
// k_iswt_lines: the last level's L line is loaded into LDS once; two LDS buffers hold the L chain, ping-ponged, and a third
// takes each level's H line: coalesced loads, 16 B per lane where aligned, the operator applied on the way.  NT threads
// work on a line (64: four lines per workgroup; 256: one), thread t takes samples t, t + NT, ... -- lanes read consecutive
// LDS addresses at every dilation, so no bank is hit twice by a wave's read.  Level 0 stores to the destination, once:
// 4 * (levels + 2) bytes of global traffic per sample with every plane kept.  LDS per workgroup: 48 KiB up to 4096 samples
// (three workgroups per CU), 96 KiB up to N1D_MAX (one).
//
// k_iswt_level: one level through global memory, one thread per output sample, any byte strides: lines beyond N1D_MAX,
// strided elements, and the cross-check of the fused kernel (option "swt_fused" = 0).  Same bits.
#include "dwt_device.h"
#include "dwt_kernels.h"
#include "dwt_line_lds.h"

namespace dwt {

namespace {

#include "dwt_band_op.h"
#include "dwt_swt_taps.h"

// the H line at `s` into LDS through operator OP: as line_to_lds, 16 B per lane where the launcher found the lines aligned
template <int OP>
static __device__ __forceinline__ void detail_to_lds(float *lds, const char *s, int N, int t, int nt, bool vec, float prm)
{
	if constexpr (OP == kBandZero) {
		for (int i = t; i < N; i += nt)
			lds[i] = 0.f;
	} else if (vec) {
		const int n4 = N >> 2;
		for (int i = t; i < n4; i += nt) {
			float4 v = *(const float4 *)(s + 16l * i);
			v.x = band_op<OP>(v.x, prm);
			v.y = band_op<OP>(v.y, prm);
			v.z = band_op<OP>(v.z, prm);
			v.w = band_op<OP>(v.w, prm);
			*(float4 *)(lds + 4 * i) = v;
		}
		for (int i = 4 * n4 + t; i < N; i += nt)
			lds[i] = band_op<OP>(*(const float *)(s + 4l * i), prm);
	} else {
		for (int i = t; i < N; i += nt)
			lds[i] = band_op<OP>(*(const float *)(s + 4l * i), prm);
	}
}

template <class F, int NT, int CAP>
__global__ __launch_bounds__(256) void k_iswt_lines(IswtLineArgs a)
{
	constexpr int LPW = 256 / NT;
	__shared__ float buf[LPW][3][CAP];
	const int sub = threadIdx.x / NT, t = threadIdx.x % NT, N = a.N;
	const long line_raw = (long)blockIdx.x * LPW + sub;
	// (a workgroup's spare lines follow the last line through every barrier and write nothing)
	const bool active = line_raw < a.n_lines;
	const long line = active ? line_raw : a.n_lines - 1;
	float *cur = buf[sub][0], *nxt = buf[sub][1], *const hb = buf[sub][2];

	line_to_lds(cur, a.src_l + line * a.src_line_stride, N, 4, t, NT, a.vec);

	for (int l = a.levels - 1; l >= 0; l--) {
		const char *const h = a.src_h + (long)l * a.plane_stride + line * a.src_line_stride;
		const float prm = a.param[l];
		switch (a.op[l]) {
		case kBandZero:
			detail_to_lds<kBandZero>(hb, h, N, t, NT, a.vec, prm);
			break;
		case kBandScale:
			detail_to_lds<kBandScale>(hb, h, N, t, NT, a.vec, prm);
			break;
		case kBandHard:
			detail_to_lds<kBandHard>(hb, h, N, t, NT, a.vec, prm);
			break;
		case kBandSoft:
			detail_to_lds<kBandSoft>(hb, h, N, t, NT, a.vec, prm);
			break;
		default:
			detail_to_lds<kBandKeep>(hb, h, N, t, NT, a.vec, prm);
			break;
		}
		__syncthreads();
		const int u = 1 << l;
		const float *const in = cur;
		float *const out = (float *)(a.dst + line * a.dst_line_stride);
		for (int p = t; p < N; p += NT) {
			const float x = iswt_point<F, int>([&](int i) { return in[i]; }, [&](int i) { return hb[i]; }, p, u, N);
			if (l > 0)
				nxt[p] = x;
			else if (active)
				out[p] = x;
		}
		__syncthreads(); // (the next level stages its H line over this one's)
		float *const q = cur;
		cur = nxt;
		nxt = q;
	}
}

template <class F>
__global__ __launch_bounds__(256) void k_iswt_level(IswtLevelArgs a)
{
	const long p = (long)blockIdx.x * 256 + threadIdx.x, N = a.N, u = 1l << a.level;
	if (p >= N)
		return;
	const int op = a.op;
	const float prm = a.param;
	for (long y = blockIdx.y; y < a.n_lines; y += gridDim.y) {
		const char *const sl = a.src_l + y * a.l_ls, *const sh = a.src_h + y * a.h_ls;
		const float x = iswt_point<F, long>([&](long i) { return *(const float *)(sl + i * 4); },
			[&](long i) { return op == kBandZero ? 0.f : band_op_on_load(op, *(const float *)(sh + i * 4), prm); }, p, u, N);
		*(float *)(a.dst + y * a.d_ls + p * a.d_es) = x;
	}
}

template <class F>
hipError_t iswt_lines_t(const IswtLineArgs &a, hipStream_t s)
{
	// the thread split of k_swt_lines: 64 threads per line up to 1024 samples, 256 above
	if (a.N <= 1024)
		k_iswt_lines<F, 64, 1024><<<(unsigned)((a.n_lines + 3l) / 4), 256, 0, s>>>(a);
	else if (a.N <= 4096)
		k_iswt_lines<F, 256, 4096><<<a.n_lines, 256, 0, s>>>(a);
	else
		k_iswt_lines<F, 256, N1D_MAX><<<a.n_lines, 256, 0, s>>>(a);
	return hipGetLastError();
}

} // namespace

hipError_t launch_iswt_lines(Wavelet w, const IswtLineArgs &a, hipStream_t s)
{
	if (a.n_lines <= 0 || a.levels <= 0)
		return hipSuccess;
	if (a.N < 1 || a.N > N1D_MAX || a.levels > SWT_MAX_LEVELS)
		return hipErrorInvalidValue;
	if (w == kCdf97S)
		return iswt_lines_t<Swt97>(a, s);
	if (w == kCdf53S)
		return iswt_lines_t<Swt53>(a, s);
	return hipErrorInvalidValue;
}

hipError_t launch_iswt_level(Wavelet w, const IswtLevelArgs &a, hipStream_t s)
{
	if (a.n_lines <= 0 || a.N <= 0)
		return hipSuccess;
	if (a.level < 0 || a.level >= SWT_MAX_LEVELS)
		return hipErrorInvalidValue;
	const dim3 grid((unsigned)((a.N + 255l) / 256), (unsigned)(a.n_lines < 65535 ? a.n_lines : 65535));
	if (w == kCdf97S)
		k_iswt_level<Swt97><<<grid, 256, 0, s>>>(a);
	else if (w == kCdf53S)
		k_iswt_level<Swt53><<<grid, 256, 0, s>>>(a);
	else
		return hipErrorInvalidValue;
	return hipGetLastError();
}

} // namespace dwt
