// dwt_timefreq.hip -- time-frequency planes on the device: the Gaussian-window STFT, the complex Morlet
// CWT and the S transform of src/gabor.c as ONE correlation of a batch of lines with a bank of complex kernels, and the
// operators the reference runs over the resulting planes (phase_derivative_s, detect_ridges{1,2,3}_s).
//
//   out(line, bin, t) = sum over i = left .. right, ascending, of x[t + i] * conj(k[center + i]),
//   left = -min(t, center), right = min(N - 1 - t, size - center - 1)                      (cdot1_s, src/gabor.c:106-138)
//
// The sum starts at +0 and rounds every product and every addition on its own (the build has -ffp-contract=off), the real
// and the imaginary part apart: x * conj(k) of a real x is (x * kr, x * -ki), so the bank's device image holds (kr, -ki)
// and each tap costs two multiplications and two additions per output.  One accumulator per output, no partial sums.
//
// k_tf_plain: one thread per output, the signal and the taps read from global memory; any strides.
// k_tf_tiled: a wave owns 512 consecutive outputs of one (line, bin), 8 per lane.  The signal window of a chunk of taps is
//   staged in LDS, zero outside [0, N): a zero sample adds (+-0, +-0) to a sum that is never -0 (it starts at +0, and x + -x
//   is +0), so running every tap over every output equals the clipped sum bit for bit while the taps are finite -- the driver
//   sends banks with an Inf or NaN tap to k_tf_plain.  That makes the tap loop wave-uniform: taps come through scalar
//   loads, 8 at a time, and meet a register window of 16 samples per lane that slides by 8 samples per 8 taps (two
//   ds_read_b128 per 64 tap-outputs).  (re, im) is one packed pair: v_pk_mul_f32 / v_pk_add_f32.
#include "dwt_kernels.h"

namespace dwt {

namespace {

typedef float v2f __attribute__((ext_vector_type(2)));

// cabsf of glibc: (float)sqrt((double)re*re + (double)im*im) -- both squares are exact in double -- with hypot's rule for
// an infinite part
__device__ __forceinline__ float tf_abs(float re, float im)
{
	if (isinf(re) || isinf(im))
		return INFINITY;
	const double d = (double)re * (double)re + (double)im * (double)im;
	return (float)sqrt(d);
}

// cargf: atan2 in double, rounded once (within half an ulp of float and a double's error of the true angle)
__device__ __forceinline__ float tf_arg(float re, float im)
{
	return (float)atan2((double)im, (double)re);
}

__device__ __forceinline__ void tf_store(const TfArgs &a, char *q, float re, float im)
{
	if (a.out == kTfComplex) {
		((float *)q)[0] = re;
		((float *)q)[1] = im;
	} else
		*(float *)q = a.out == kTfAbs ? tf_abs(re, im) : tf_arg(re, im);
}

__global__ __launch_bounds__(256) void k_tf_plain(TfArgs a)
{
	const long t = a.t0 + (long)blockIdx.x * 256 + threadIdx.x;
	if (t >= (long)a.t0 + a.nt)
		return;
	for (int b = blockIdx.y; b < a.n_bins; b += gridDim.y) {
		const TfBin bin = a.bins[b];
		const float2 *const k = a.taps + bin.off + bin.center;
		const long left = -(t < bin.center ? t : (long)bin.center);
		const long right = a.N - 1 - t < bin.size - bin.center - 1 ? a.N - 1 - t : (long)bin.size - bin.center - 1;
		for (int y = blockIdx.z; y < a.n_lines; y += gridDim.z) {
			const char *const s = a.src + y * a.src_ls + t * a.src_es;
			float re = 0.f, im = 0.f;
			for (long i = left; i <= right; i++) {
				const float x = *(const float *)(s + i * a.src_es);
				const float2 c = k[i];
				re = re + x * c.x;
				im = im + x * c.y;
			}
			tf_store(a, a.dst + y * a.plane_stride + bin.row * a.row_stride + (t - a.t0) * a.dst_es, re, im);
		}
	}
}

constexpr int TF_R = 8;              // outputs per lane
constexpr int TF_TILE = 64 * TF_R;   // outputs per wave
constexpr int TF_KC = 512;           // taps per staged window (a multiple of TF_R)
constexpr int TF_WIN = TF_TILE + TF_KC + TF_R;

// eight samples of the lane's window into w[at ..] (element by element: w stays in registers)
__device__ __forceinline__ void tf_window(float (&w)[2 * TF_R], int at, float4 lo, float4 hi)
{
	w[at + 0] = lo.x, w[at + 1] = lo.y, w[at + 2] = lo.z, w[at + 3] = lo.w;
	w[at + 4] = hi.x, w[at + 5] = hi.y, w[at + 6] = hi.z, w[at + 7] = hi.w;
}

// taps j .. j+TF_R-1 (GUARD: those below `rem` only) over the lane's 8 outputs: w[r + jj] is the sample of output r at tap jj
template <bool GUARD>
__device__ __forceinline__ void tf_group(v2f (&acc)[TF_R], const float (&w)[2 * TF_R], const v2f *__restrict__ k, int rem)
{
#pragma unroll
	for (int jj = 0; jj < TF_R; jj++) {
		if (GUARD && jj >= rem)
			break;
		const v2f c = k[jj];
#pragma unroll
		for (int r = 0; r < TF_R; r++) {
			const v2f x = {w[r + jj], w[r + jj]};
			acc[r] = acc[r] + x * c;
		}
	}
}

// (the bank's arrays come as __restrict__ parameters of their own: that is what lets the compiler prove that no store of the
// kernel changes them, and fetch bins and taps through the scalar cache)
__global__ __launch_bounds__(64) void k_tf_tiled(TfArgs a, const v2f *__restrict__ bank_taps, const TfBin *__restrict__ bank_bins,
	const int *__restrict__ bank_order)
{
	__shared__ __attribute__((aligned(16))) float win[TF_WIN];
	const int lane = threadIdx.x;
	const long T0 = a.t0 + (long)blockIdx.x * TF_TILE; // first output of the tile
	const long t_end = (long)a.t0 + a.nt;
	for (int rank = blockIdx.z; rank < a.n_bins; rank += gridDim.z) {
		const TfBin bin = bank_bins[bank_order[rank]];
		const v2f *const taps = bank_taps + bin.off;
		for (int y = blockIdx.y; y < a.n_lines; y += gridDim.y) {
			const float *const s = (const float *)(a.src + y * a.src_ls);
			v2f acc[TF_R];
#pragma unroll
			for (int r = 0; r < TF_R; r++)
				acc[r] = (v2f){0.f, 0.f};
			for (int j0 = 0; j0 < bin.size; j0 += TF_KC) {
				const int kc = bin.size - j0 < TF_KC ? bin.size - j0 : TF_KC;
				// window sample i is x[T0 - center + j0 + i]
				const long p0 = T0 - bin.center + j0;
				__syncthreads();
				for (int i = lane; i < TF_WIN; i += 64) {
					const long p = p0 + i;
					win[i] = p >= 0 && p < a.N ? s[p] : 0.f;
				}
				__syncthreads();
				const float4 *const wl = (const float4 *)(win + lane * TF_R);
				float w[2 * TF_R];
				tf_window(w, 0, wl[0], wl[1]);
				const v2f *k = taps + j0;
				int g = 0;
				for (; g + TF_R <= kc; g += TF_R) {
					tf_window(w, TF_R, wl[g / 4 + 2], wl[g / 4 + 3]);
					tf_group<false>(acc, w, k + g, TF_R);
#pragma unroll
					for (int r = 0; r < TF_R; r++)
						w[r] = w[r + TF_R];
				}
				if (g < kc) {
					tf_window(w, TF_R, wl[g / 4 + 2], wl[g / 4 + 3]);
					tf_group<true>(acc, w, k + g, kc - g);
				}
			}
			char *const q = a.dst + y * a.plane_stride + bin.row * a.row_stride;
#pragma unroll
			for (int r = 0; r < TF_R; r++) {
				const long t = T0 + lane * TF_R + r;
				if (t < t_end)
					tf_store(a, q + (t - a.t0) * a.dst_es, acc[r].x, acc[r].y);
			}
		}
	}
}

__device__ __forceinline__ float at(const char *p, long y, long x, const TfPlaneArgs &a)
{
	return *(const float *)(p + y * a.sx + x * a.sy);
}

// 1 if the sample is no smaller than its neighbour in the direction of the gradient (grad_max_s, src/gabor.c:1020-1109):
// the angle is atan2 of the central differences, the direction its cosine and sine compared with -+1/2.  The angle is
// taken in double and rounded once, cosine and sine likewise.
__device__ __forceinline__ bool grad_max(const char *p, long y, long x, const TfPlaneArgs &a)
{
	const float dx = (at(p, y, x + 1, a) - at(p, y, x - 1, a)) / 2.f;
	const float dy = (at(p, y + 1, x, a) - at(p, y - 1, x, a)) / 2.f;
	const float angle = (float)atan2((double)dy, (double)dx);
	const float dir_x = 1.f * (float)cos((double)angle), dir_y = 1.f * (float)sin((double)angle);
	const int nx = dir_x < -0.5f ? -1 : dir_x > 0.5f ? 1 : 0;
	const int ny = dir_y < -0.5f ? -1 : dir_y > 0.5f ? 1 : 0;
	return at(p, y, x, a) >= at(p, y + ny, x + nx, a);
}

__global__ __launch_bounds__(256) void k_tf_plane_op(TfPlaneArgs a)
{
	const long x = (long)blockIdx.x * 256 + threadIdx.x;
	if (x >= a.size_x)
		return;
	const float two_pi = 2.f * (float)M_PI;
	for (int pl = blockIdx.z; pl < a.n_planes; pl += gridDim.z) {
		const char *const p = a.src + pl * a.ps;
		for (long y = blockIdx.y; y < a.size_y; y += gridDim.y) {
			float v = 0.f;
			if (a.op == 0) {
				if (x > 0) {
					v = -at(p, y, x - 1, a) + at(p, y, x, a);
					// (the reference's loops never end on a value that the step does not move; such a value stays)
					while (v > a.param) {
						const float n = v - two_pi;
						if (n == v)
							break;
						v = n;
					}
					while (v < -a.param) {
						const float n = v + two_pi;
						if (n == v)
							break;
						v = n;
					}
				}
			} else if (x > 0 && x < a.size_x - 1) {
				const float m = at(p, y, x, a);
				if (a.op == 1) {
					const float m0 = at(p, y, x - 1, a), m2 = at(p, y, x + 1, a);
					const float f = -1.f * (m0 - m) * (m - m2);
					if (f > 0.f && m > a.param)
						v = m / 2.f / (float)M_PI;
				} else if (a.op == 2) {
					if (m < 0.f && fabsf(m) > a.param)
						v = fabsf(m) / 2.f / (float)M_PI;
				} else if (y > 0 && y < a.size_y - 1) {
					if (grad_max(p, y, x, a) && m > a.param)
						v = m / 2.f / (float)M_PI;
				}
			}
			*(float *)(a.dst + pl * a.ps + y * a.sx + x * a.sy) = v;
		}
	}
}

unsigned capped(long n) { return (unsigned)(n < 65535 ? n : 65535); } // (past the cap: tests/test_hip_grid_limits.py)

} // namespace

hipError_t launch_tf_plain(const TfArgs &a, hipStream_t s)
{
	if (a.n_lines <= 0 || a.nt <= 0 || a.n_bins <= 0)
		return hipSuccess;
	const dim3 grid((unsigned)((a.nt + 255l) / 256), capped(a.n_bins), capped(a.n_lines));
	k_tf_plain<<<grid, 256, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_tf_tiled(const TfArgs &a, hipStream_t s)
{
	if (a.n_lines <= 0 || a.nt <= 0 || a.n_bins <= 0)
		return hipSuccess;
	if (a.src_es != 4 || a.src_ls % 4 || (uintptr_t)a.src % 4)
		return hipErrorInvalidValue;
	// z (the slowest index of the dispatch order) walks the bins from the longest kernel down
	const dim3 grid((unsigned)((a.nt + (long)TF_TILE - 1) / TF_TILE), capped(a.n_lines), capped(a.n_bins));
	k_tf_tiled<<<grid, 64, 0, s>>>(a, (const v2f *)a.taps, a.bins, a.order);
	return hipGetLastError();
}

hipError_t launch_tf_plane_op(const TfPlaneArgs &a, hipStream_t s)
{
	if (a.n_planes <= 0 || a.size_x <= 0 || a.size_y <= 0)
		return hipSuccess;
	if (a.op < 0 || a.op > 3)
		return hipErrorInvalidValue;
	const dim3 grid((unsigned)((a.size_x + 255l) / 256), capped(a.size_y), capped(a.n_planes));
	k_tf_plane_op<<<grid, 256, 0, s>>>(a);
	return hipGetLastError();
}

} // namespace dwt
