// dwt_swt2d.hip -- the stationary (undecimated) wavelet transform of image batches, one level per launch (gfx950).
//
// A level at dilation u = 1 << level is the reference's row function (swt_cdf97_f_ex_stride_s / swt_cdf53_f_ex_stride_s,
// src/swt.c; dwt_swt_taps.h) run along x for every row of the level's input A and then along y for every column:
//
//     Lr = conv_x(A, g_low)   Hr = conv_x(A, g_high)
//     LL = conv_y(Lr, g_low)  LH = conv_y(Lr, g_high)  HL = conv_y(Hr, g_low)  HH = conv_y(Hr, g_high)
//
// every conv the tap sum of dwt_swt_taps.h (float32, product and sum rounded separately, from +0.0f, borders replicated).
// No direction is skipped: a 1-row image takes its column pass with N = 1.  Every plane is W x H.
//
// k_swt2d_fused: dense device images, dilations 1 .. 16.  A workgroup of 256 lanes owns SWT2D_TILE_W contiguous columns
// and SWT2D_TILE_H rows of the level's ROW LATTICE r0 + u*i (r0 = residue + u*i0): the vertical filter of those rows
// reads rows r0 + u*(i - k) only, so TILE_H + 2c input rows serve the tile at ANY dilation (a tile of adjacent rows would
// need TILE_H + 2cu).  LDS slot j holds row B(r0 + u*(j - c)) with B the border rule (SwtClamp, or SwtReflect for the
// invertible transform of DESIGN.md s29): tap k of output row i needs row B(r0 + u*i - u*k) = B(r0 + u*((i + c - k) - c)),
// which is slot i + c - k by the slot rule itself, whatever B is -- with its c*u columns of halo on both sides, addresses
// mapped by B per element; only the raw input is staged.  One barrier.  Then a lane owns one column and marches down the slots: 2c+1
// LDS reads (consecutive lanes, consecutive addresses at every dilation) give Lr and Hr of the slot, which enter a
// register window of 2c+1 pairs (Lr, Hr) indexed at compile time; once the window is full every new slot emits one
// output row: (LL, HL) is one packed sum under g_low and (LH, HH) one under g_high (v_pk_mul_f32 / v_pk_add_f32), four
// coalesced 4-byte stores.  The input is read once (plus the halo), the four planes are written once.
//
// k_swt2d_rows / k_swt2d_cols: the same level as two launches through global memory, one thread per output sample, any
// byte strides, Lr and Hr in library scratch: strided elements, deeper levels, and the cross-check of the fused kernel
// (option "swt2d_fused" = 0).  Same bits.
#include "dwt_device.h"
#include "dwt_kernels.h"

namespace dwt {

namespace {

#include "dwt_swt_taps.h"

typedef float v2f __attribute__((ext_vector_type(2)));

constexpr int TW = SWT2D_TILE_W, TH = SWT2D_TILE_H;
static_assert(TW == 256, "one column per lane of the workgroup");

// rows of the lattice class of residue 0 (the longest), and the tiles that cover one class
static __host__ __device__ inline int lattice_rows(int H, int level) { return (int)((H + (1l << level) - 1) >> level); }
static __host__ __device__ inline int class_tiles(int H, int level) { return (lattice_rows(H, level) + TH - 1) / TH; }

template <class F, class B>
__global__ __launch_bounds__(256, 4) void k_swt2d_fused(Swt2dLevelArgs a)
{
	constexpr int C = F::CL, NW = 2 * C + 1;
	extern __shared__ float tile[]; // (n_out + 2C) rows of TW + 2*C*u floats
	const int u = 1 << a.level, W = a.W, H = a.H, halo = C * u, pitch = TW + 2 * halo;
	const int tiles = class_tiles(H, a.level);
	const int x0 = blockIdx.x * TW, res = blockIdx.y / tiles, i0 = (blockIdx.y % tiles) * TH;
	const int r0 = res + u * i0; // (u <= 16, i0 <= H / u + TH: inside int)
	if (r0 >= H)
		return; // the shorter classes' spare tiles (the whole workgroup)
	const int n_out = min(TH, (H - r0 + u - 1) / u), n_slots = n_out + 2 * C;
	const char *const s = a.src + (long)blockIdx.z * a.src_bs;
	const int t = threadIdx.x;

	for (int j = 0; j < n_slots; j++) {
		const long r = B::map((long)r0 + (long)u * (j - C), (long)H);
		const float *const row = (const float *)(s + r * a.src_sx);
		for (int m = t; m < pitch; m += 256) {
			const int c = B::map(x0 - halo + m, W);
			tile[j * pitch + m] = row[c];
		}
	}
	__syncthreads();

	const int x = x0 + t;
	const bool live = x < W; // (a spare lane computes on replicated columns and stores nothing)
	// the lane's four output pointers walk down the lattice rows
	const long d_off = (long)blockIdx.z * a.d_bs + (long)r0 * a.d_sx + 4l * x, d_step = (long)u * a.d_sx, ll_step = (long)u * a.ll_sx;
	char *hl = a.hl + d_off, *lh = a.lh + d_off, *hh = a.hh + d_off;
	char *ll = a.ll ? a.ll + (long)blockIdx.z * a.ll_bs + (long)r0 * a.ll_sx + 4l * x : nullptr;
	v2f win[NW]; // slot j at win[j % NW]
	for (int jb = 0; jb < n_slots; jb += NW) {
#pragma unroll
		for (int q = 0; q < NW; q++) {
			const int j = jb + q;
			if (j < n_slots) { // (uniform)
				const float *const in = tile + j * pitch + halo + t;
				float v[NW], lo, hi;
#pragma unroll
				for (int k = -C; k <= C; k++)
					v[k + C] = in[-u * k];
				swt_sums<F, float>(v, &lo, &hi);
				win[q] = v2f{lo, hi};
			}
			if (j >= 2 * C && j < n_slots) {
				// output row i = j - 2C: tap k reads slot i + C - k = j - (k + C)
				v2f p[NW], l2, h2;
#pragma unroll
				for (int m = 0; m < NW; m++)
					p[m] = win[(q - m + NW) % NW];
				swt_sums<F, v2f>(p, &l2, &h2);
				if (live) {
					if (ll)
						*(float *)ll = l2.x;
					*(float *)hl = l2.y;
					*(float *)lh = h2.x;
					*(float *)hh = h2.y;
				}
				hl += d_step, lh += d_step, hh += d_step;
				if (ll)
					ll += ll_step;
			}
		}
	}
}

// the two passes through global memory: thread (x, q) with q = b*H + y over grid.y
template <class F, class B>
__global__ __launch_bounds__(256) void k_swt2d_rows(Swt2dLevelArgs a)
{
	const long x = (long)blockIdx.x * 256 + threadIdx.x, W = a.W, H = a.H, u = 1l << a.level;
	if (x >= W)
		return;
	for (long q = blockIdx.y; q < H * a.batch; q += gridDim.y) {
		const long b = q / H, y = q % H;
		const char *const s = a.src + b * a.src_bs + y * a.src_sx;
		const long es = a.src_sy;
		float lo, hi;
		swt_point<F, long, B>([&](long i) { return *(const float *)(s + i * es); }, x, u, W, &lo, &hi);
		*(float *)(a.lr + (q * W + x) * 4) = lo;
		*(float *)(a.hr + (q * W + x) * 4) = hi;
	}
}

template <class F, class B>
__global__ __launch_bounds__(256) void k_swt2d_cols(Swt2dLevelArgs a)
{
	const long x = (long)blockIdx.x * 256 + threadIdx.x, W = a.W, H = a.H, u = 1l << a.level;
	if (x >= W)
		return;
	for (long q = blockIdx.y; q < H * a.batch; q += gridDim.y) {
		const long b = q / H, y = q % H;
		const char *const lr = a.lr + (b * H * W + x) * 4, *const hr = a.hr + (b * H * W + x) * 4;
		float ll, lh, hl, hh;
		swt_point<F, long, B>([&](long i) { return *(const float *)(lr + i * W * 4); }, y, u, H, &ll, &lh);
		swt_point<F, long, B>([&](long i) { return *(const float *)(hr + i * W * 4); }, y, u, H, &hl, &hh);
		const long off = b * a.d_bs + y * a.d_sx + x * a.d_sy;
		if (a.ll)
			*(float *)(a.ll + b * a.ll_bs + y * a.ll_sx + x * a.d_sy) = ll;
		*(float *)(a.hl + off) = hl;
		*(float *)(a.lh + off) = lh;
		*(float *)(a.hh + off) = hh;
	}
}

static bool border_ok(const Swt2dLevelArgs &a) { return a.border == kSwtReplicate || a.border == kSwtSymmetric; }
static bool pass_args_ok(const Swt2dLevelArgs &a) { return a.level >= 0 && a.level < SWT_MAX_LEVELS && a.lr && a.hr && a.hl && a.lh && a.hh && border_ok(a); }
static dim3 pass_grid(const Swt2dLevelArgs &a)
{
	const long lines = (long)a.H * a.batch;
	return dim3((unsigned)((a.W + 255l) / 256), (unsigned)(lines < 65535 ? lines : 65535)); // (past the cap: tests/test_hip_grid_limits.py)
}

template <class F, class B>
hipError_t swt2d_fused_t(const Swt2dLevelArgs &a, hipStream_t s)
{
	const int rows = std::min(TH, lattice_rows(a.H, a.level)) + 2 * F::CL;
	const size_t lds = (size_t)rows * (TW + 2 * F::CL * (1 << a.level)) * sizeof(float);
	if (hipError_t e = allow_lds((const void *)k_swt2d_fused<F, B>, lds))
		return e;
	const long classes = std::min<long>(1l << a.level, a.H);
	const dim3 grid((unsigned)((a.W + TW - 1l) / TW), (unsigned)(classes * class_tiles(a.H, a.level)), (unsigned)a.batch);
	k_swt2d_fused<F, B><<<grid, 256, lds, s>>>(a);
	return hipGetLastError();
}

} // namespace

bool swt2d_fused_fits(const Swt2dLevelArgs &a)
{
	if (a.level < 0 || a.level >= SWT2D_FUSED_LEVELS || a.src_sy != 4 || a.d_sy != 4 || a.batch > 65535) // (past the cap: tests/test_hip_grid_limits.py)
		return false;
	return std::min<long>(1l << a.level, a.H) * class_tiles(a.H, a.level) <= 65535;
}

hipError_t launch_swt2d_fused(Wavelet w, const Swt2dLevelArgs &a, hipStream_t s)
{
	if (a.batch <= 0 || a.W <= 0 || a.H <= 0)
		return hipSuccess;
	if (!swt2d_fused_fits(a) || !a.hl || !a.lh || !a.hh || !border_ok(a))
		return hipErrorInvalidValue;
	if (w == kCdf97S)
		return a.border ? swt2d_fused_t<Swt97, SwtReflect>(a, s) : swt2d_fused_t<Swt97, SwtClamp>(a, s);
	if (w == kCdf53S)
		return a.border ? swt2d_fused_t<Swt53, SwtReflect>(a, s) : swt2d_fused_t<Swt53, SwtClamp>(a, s);
	return hipErrorInvalidValue;
}

hipError_t launch_swt2d_rows(Wavelet w, const Swt2dLevelArgs &a, hipStream_t s)
{
	if (a.batch <= 0 || a.W <= 0 || a.H <= 0)
		return hipSuccess;
	if (!pass_args_ok(a))
		return hipErrorInvalidValue;
	if (w == kCdf97S && a.border)
		k_swt2d_rows<Swt97, SwtReflect><<<pass_grid(a), 256, 0, s>>>(a);
	else if (w == kCdf97S)
		k_swt2d_rows<Swt97, SwtClamp><<<pass_grid(a), 256, 0, s>>>(a);
	else if (w == kCdf53S && a.border)
		k_swt2d_rows<Swt53, SwtReflect><<<pass_grid(a), 256, 0, s>>>(a);
	else if (w == kCdf53S)
		k_swt2d_rows<Swt53, SwtClamp><<<pass_grid(a), 256, 0, s>>>(a);
	else
		return hipErrorInvalidValue;
	return hipGetLastError();
}

hipError_t launch_swt2d_cols(Wavelet w, const Swt2dLevelArgs &a, hipStream_t s)
{
	if (a.batch <= 0 || a.W <= 0 || a.H <= 0)
		return hipSuccess;
	if (!pass_args_ok(a))
		return hipErrorInvalidValue;
	if (w == kCdf97S && a.border)
		k_swt2d_cols<Swt97, SwtReflect><<<pass_grid(a), 256, 0, s>>>(a);
	else if (w == kCdf97S)
		k_swt2d_cols<Swt97, SwtClamp><<<pass_grid(a), 256, 0, s>>>(a);
	else if (w == kCdf53S && a.border)
		k_swt2d_cols<Swt53, SwtReflect><<<pass_grid(a), 256, 0, s>>>(a);
	else if (w == kCdf53S)
		k_swt2d_cols<Swt53, SwtClamp><<<pass_grid(a), 256, 0, s>>>(a);
	else
		return hipErrorInvalidValue;
	return hipGetLastError();
}

} // namespace dwt
