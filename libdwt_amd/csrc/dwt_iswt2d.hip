// dwt_iswt2d.hip -- the inverse stationary wavelet transform of image batches under the symmetric border, one level per
// launch (gfx950).  An extension: the reference stops at the forward functions.
//
// A level at dilation u = 1 << level undoes the forward level (dwt_swt2d.hip) in the reverse order, columns first:
//
//     Lr = 0.5f * (conv_y(LL, sl) + conv_y(LH, sh))   Hr = 0.5f * (conv_y(HL, sl) + conv_y(HH, sh))
//     A  = 0.5f * (conv_x(Lr, sl) + conv_x(Hr, sh))
//
// every conv the tap sum of dwt_swt_taps.h over whole-sample reflected indices (float32, every product and sum rounded on
// its own, from +0.0f), sl and sh the synthesis filters there.  HL, LH and HH pass through their band operators (KEEP,
// ZERO, SCALE, HARD, SOFT; dwt_band_op.h) as they are read; a ZERO plane is never read.  No direction is skipped.
//
// k_iswt2d_fused: dense device planes, dilations 1 .. 16.  A workgroup of 256 lanes owns ISWT2D_TILE_W contiguous output
// columns and `th` rows of the level's ROW LATTICE r0 + u*i, as the forward kernel does: the column filter of those rows
// reads rows r0 + u*(i - k) only, so th + 2c rows of each plane serve the tile at ANY dilation.  Phase 1: a lane owns one
// of the tile's TILE_W + 2cu columns (the c*u halo columns on both sides are computed too, at reflected column indices) and
// marches down the slots j, slot j being row reflect(r0 + u*(j - c)): four coalesced 4-byte loads straight from global
// memory enter two register windows of 2c+1 pairs, (LL, HL) and (LH, HH), indexed at compile time; once the windows are
// full every new slot gives one pair (Lr, Hr) -- one packed sum under sl and one under sh -- which goes to LDS.  One
// barrier.  Phase 2: a lane owns one output column and filters each of the th rows of Lr and Hr out of LDS (consecutive
// lanes, consecutive addresses at every dilation: no bank is hit twice), one coalesced 4-byte store per row.  The four
// planes are read once (plus the halos), the output is written once: 20 bytes per sample and level, against 36 for the
// two passes below.  LDS is 2 * th * (TILE_W + 2cu) floats: th is 32 while that stays under 80 KiB and 16 above, so two
// workgroups always share a CU.
//
// k_iswt2d_cols / k_iswt2d_rows: the same level as two launches through global memory, one thread per output sample, Lr
// and Hr in library scratch, any destination strides: deeper levels, strided destinations, and the cross-check of the
// fused kernel (option "swt2d_fused" = 0).  Same bits.
#include "dwt_device.h"
#include "dwt_kernels.h"

namespace dwt {

namespace {

#include "dwt_band_op.h"
#include "dwt_swt_taps.h"

typedef float v2f __attribute__((ext_vector_type(2)));

constexpr int TW = ISWT2D_TILE_W;
static_assert(TW == 256, "one output column per lane of the workgroup");

// rows of the tile: 32 while Lr and Hr of 32 rows stay under 80 KiB of LDS (two workgroups per CU), 16 above
template <class F>
static __host__ __device__ inline int tile_rows(int level)
{
	return 2l * 32 * (TW + 2 * F::CL * (1 << level)) * 4 < (80l << 10) ? 32 : 16;
}
// rows of the lattice class of residue 0 (the longest), and the tiles that cover one class
static __host__ __device__ inline int lattice_rows(int H, int level) { return (int)((H + (1l << level) - 1) >> level); }
static __host__ __device__ inline int class_tiles(int H, int level, int th) { return (lattice_rows(H, level) + th - 1) / th; }

static __device__ __forceinline__ float detail(const char *p, int op, float prm)
{
	return op == kBandZero ? 0.f : band_op_on_load(op, *(const float *)p, prm);
}

template <class F>
__global__ __launch_bounds__(256, 2) void k_iswt2d_fused(Iswt2dLevelArgs a)
{
	constexpr int C = F::CL, CH = F::CH, NW = 2 * C + 1;
	extern __shared__ float tile[]; // Lr, then Hr: th rows of TW + 2*C*u floats each
	const int u = 1 << a.level, W = a.W, H = a.H, halo = C * u, pitch = TW + 2 * halo, th = tile_rows<F>(a.level);
	const int tiles = class_tiles(H, a.level, th);
	const int x0 = blockIdx.x * TW, res = blockIdx.y / tiles, i0 = (blockIdx.y % tiles) * th;
	const int r0 = res + u * i0; // (u <= 16, i0 <= H / u + th: inside int)
	if (r0 >= H)
		return; // the shorter classes' spare tiles (the whole workgroup)
	const int n_out = min(th, (H - r0 + u - 1) / u), n_slots = n_out + 2 * C;
	float *const lr = tile, *const hr = tile + th * pitch;
	const long b = blockIdx.z;
	const char *const ll = a.ll + b * a.ll_bs, *const hl = a.hl + b * a.d_bs, *const lh = a.lh + b * a.d_bs, *const hh = a.hh + b * a.d_bs;
	const int op_hl = a.op[0], op_lh = a.op[1], op_hh = a.op[2];
	const float p_hl = a.param[0], p_lh = a.param[1], p_hh = a.param[2];
	const int t = threadIdx.x;

	for (int m = t; m < pitch; m += 256) {
		const long c4 = 4l * SwtReflect::map(x0 - halo + m, W);
		v2f wl[NW], wh[NW]; // (LL, HL) and (LH, HH) of slot j at [j % NW]
		for (int jb = 0; jb < n_slots; jb += NW) {
#pragma unroll
			for (int q = 0; q < NW; q++) {
				const int j = jb + q;
				if (j < n_slots) { // (uniform)
					const long r = SwtReflect::map((long)r0 + (long)u * (j - C), (long)H);
					const long off = r * a.d_sx + c4;
					wl[q] = v2f{*(const float *)(ll + r * a.ll_sx + c4), detail(hl + off, op_hl, p_hl)};
					wh[q] = v2f{detail(lh + off, op_lh, p_lh), detail(hh + off, op_hh, p_hh)};
				}
				if (j >= 2 * C && j < n_slots) {
					// output row i = j - 2C: tap k reads slot i + C - k = j - (k + C)
					v2f pl[NW], ph[NW];
#pragma unroll
					for (int k = 0; k < NW; k++) {
						pl[k] = wl[(q - k + NW) % NW];
						ph[k] = wh[(q - k + NW) % NW];
					}
					const v2f o = iswt_sums<F, v2f>(pl, ph);
					lr[(j - 2 * C) * pitch + m] = o.x;
					hr[(j - 2 * C) * pitch + m] = o.y;
				}
			}
		}
	}
	__syncthreads();

	const int x = x0 + t;
	const bool live = x < W; // (a spare lane filters reflected columns and stores nothing)
	char *out = a.dst + b * a.dst_bs + (long)r0 * a.dst_sx + 4l * x;
	const long step = (long)u * a.dst_sx;
	for (int i = 0; i < n_out; i++, out += step) {
		const float *const pl = lr + i * pitch + halo + t, *const ph = hr + i * pitch + halo + t;
		float vl[NW], vh[NW];
#pragma unroll
		for (int k = -C; k <= C; k++) {
			vh[k + C] = ph[-u * k];
			vl[k + C] = (k >= -CH && k <= CH) ? pl[-u * k] : 0.f;
		}
		const float o = iswt_sums<F, float>(vl, vh);
		if (live)
			*(float *)out = o;
	}
}

// the two passes through global memory: thread (x, q) with q = b*H + y over grid.y
template <class F>
__global__ __launch_bounds__(256) void k_iswt2d_cols(Iswt2dLevelArgs a)
{
	const long x = (long)blockIdx.x * 256 + threadIdx.x, W = a.W, H = a.H, u = 1l << a.level;
	if (x >= W)
		return;
	const int op_hl = a.op[0], op_lh = a.op[1], op_hh = a.op[2];
	const float p_hl = a.param[0], p_lh = a.param[1], p_hh = a.param[2];
	for (long q = blockIdx.y; q < H * a.batch; q += gridDim.y) {
		const long b = q / H, y = q % H, d = b * a.d_bs + x * 4;
		const char *const ll = a.ll + b * a.ll_bs + x * 4, *const hl = a.hl + d, *const lh = a.lh + d, *const hh = a.hh + d;
		const long lsx = a.ll_sx, dsx = a.d_sx;
		const float lo = iswt_point<F, long>([&](long i) { return *(const float *)(ll + i * lsx); },
			[&](long i) { return detail(lh + i * dsx, op_lh, p_lh); }, y, u, H);
		const float hi = iswt_point<F, long>([&](long i) { return detail(hl + i * dsx, op_hl, p_hl); },
			[&](long i) { return detail(hh + i * dsx, op_hh, p_hh); }, y, u, H);
		*(float *)(a.lr + (q * W + x) * 4) = lo;
		*(float *)(a.hr + (q * W + x) * 4) = hi;
	}
}

template <class F>
__global__ __launch_bounds__(256) void k_iswt2d_rows(Iswt2dLevelArgs a)
{
	const long x = (long)blockIdx.x * 256 + threadIdx.x, W = a.W, H = a.H, u = 1l << a.level;
	if (x >= W)
		return;
	for (long q = blockIdx.y; q < H * a.batch; q += gridDim.y) {
		const long b = q / H, y = q % H;
		const char *const lr = a.lr + q * W * 4, *const hr = a.hr + q * W * 4;
		const float o = iswt_point<F, long>([&](long i) { return *(const float *)(lr + i * 4); }, [&](long i) { return *(const float *)(hr + i * 4); }, x, u, W);
		*(float *)(a.dst + b * a.dst_bs + y * a.dst_sx + x * a.dst_sy) = o;
	}
}

static bool pass_args_ok(const Iswt2dLevelArgs &a)
{
	return a.level >= 0 && a.level < SWT_MAX_LEVELS && a.lr && a.hr && a.ll && a.hl && a.lh && a.hh && a.dst;
}
static dim3 pass_grid(const Iswt2dLevelArgs &a)
{
	const long lines = (long)a.H * a.batch;
	return dim3((unsigned)((a.W + 255l) / 256), (unsigned)(lines < 65535 ? lines : 65535));
}

template <class F>
static long fused_grid_y(const Iswt2dLevelArgs &a)
{
	return std::min<long>(1l << a.level, a.H) * class_tiles(a.H, a.level, tile_rows<F>(a.level));
}

template <class F>
hipError_t iswt2d_fused_t(const Iswt2dLevelArgs &a, hipStream_t s)
{
	const size_t lds = (size_t)2 * tile_rows<F>(a.level) * (TW + 2 * F::CL * (1 << a.level)) * sizeof(float);
	if (hipError_t e = allow_lds((const void *)k_iswt2d_fused<F>, lds))
		return e;
	const dim3 grid((unsigned)((a.W + TW - 1l) / TW), (unsigned)fused_grid_y<F>(a), (unsigned)a.batch);
	k_iswt2d_fused<F><<<grid, 256, lds, s>>>(a);
	return hipGetLastError();
}

} // namespace

bool iswt2d_fused_fits(const Iswt2dLevelArgs &a)
{
	if (a.level < 0 || a.level >= ISWT2D_FUSED_LEVELS || a.dst_sy != 4 || a.batch > 65535)
		return false;
	return fused_grid_y<Swt97>(a) <= 65535; // (the 9/7 tiles are never taller than the 5/3 ones: the larger count)
}

hipError_t launch_iswt2d_fused(Wavelet w, const Iswt2dLevelArgs &a, hipStream_t s)
{
	if (a.batch <= 0 || a.W <= 0 || a.H <= 0)
		return hipSuccess;
	if (!iswt2d_fused_fits(a) || !a.ll || !a.hl || !a.lh || !a.hh || !a.dst)
		return hipErrorInvalidValue;
	if (w == kCdf97S)
		return iswt2d_fused_t<Swt97>(a, s);
	if (w == kCdf53S)
		return iswt2d_fused_t<Swt53>(a, s);
	return hipErrorInvalidValue;
}

hipError_t launch_iswt2d_cols(Wavelet w, const Iswt2dLevelArgs &a, hipStream_t s)
{
	if (a.batch <= 0 || a.W <= 0 || a.H <= 0)
		return hipSuccess;
	if (!pass_args_ok(a))
		return hipErrorInvalidValue;
	if (w == kCdf97S)
		k_iswt2d_cols<Swt97><<<pass_grid(a), 256, 0, s>>>(a);
	else if (w == kCdf53S)
		k_iswt2d_cols<Swt53><<<pass_grid(a), 256, 0, s>>>(a);
	else
		return hipErrorInvalidValue;
	return hipGetLastError();
}

hipError_t launch_iswt2d_rows(Wavelet w, const Iswt2dLevelArgs &a, hipStream_t s)
{
	if (a.batch <= 0 || a.W <= 0 || a.H <= 0)
		return hipSuccess;
	if (!pass_args_ok(a))
		return hipErrorInvalidValue;
	if (w == kCdf97S)
		k_iswt2d_rows<Swt97><<<pass_grid(a), 256, 0, s>>>(a);
	else if (w == kCdf53S)
		k_iswt2d_rows<Swt53><<<pass_grid(a), 256, 0, s>>>(a);
	else
		return hipErrorInvalidValue;
	return hipGetLastError();
}

} // namespace dwt
