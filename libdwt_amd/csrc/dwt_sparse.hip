// dwt_sparse.hip -- sparse coefficient streams ON THE DEVICE: the kept elements of dense Mallat frames (binary32, binary16,
// int16, int32) packed into (position, value) entries in stream order -- bands coarse to fine, raster order inside a band
// --, and scattered back.  include/libdwt_hip.h states the format; DESIGN.md s32 the kernels.
//
// A frame is cut into tiles: SPARSE_TILE_SAMPLES consecutive samples of one band's raster order, enumerated in stream
// order (dwt_sparse_geom.c).  A workgroup takes a tile.  The tile's rows are walked by 16-byte chunks of the FRAME's
// columns (so that a chunk is one aligned access wherever the planes are 16-byte aligned), 256 chunks per trip, chunk by
// chunk in raster order; a lane masks the samples of its chunk that lie outside the band or outside the tile.
//   k_sparse_tiles<ES, false>  launch 1: the tile's kept elements -> tile[b][t].
//   k_sparse_scan              launch 2: one workgroup per frame scans tile[b][*] exclusively, in place, and writes the
//                              frame's offsets: the first entry of every band's first tile, and the total.
//   k_sparse_tiles<ES, true>   launch 3: the same walk; an entry goes to tile[b][t] + its rank in the tile, the rank from
//                              the 64-bit ballots of the lanes' samples, mbcnt and a prefix over the four waves in LDS.
//                              The capacity is checked per entry.
//   k_sparse_zero, k_sparse_scatter  the way back: zero bits into every own element, then the entries.
// The order is fixed by construction: no atomics, no workgroup waits for another.  No arithmetic on the values.
#include "dwt_device.h"
#include "dwt_runs.h"

#include <algorithm>

namespace dwt {

namespace {

template <int ES>
static __device__ __forceinline__ unsigned elem_load(const char *p)
{
	if constexpr (ES == 2)
		return *(const unsigned short *)p;
	else
		return *(const unsigned *)p;
}
template <int ES>
static __device__ __forceinline__ void elem_store(char *p, unsigned v)
{
	if constexpr (ES == 2)
		*(unsigned short *)p = (unsigned short)v;
	else
		*(unsigned *)p = v;
}

template <int ES, bool PACK>
__global__ __launch_bounds__(256) void k_sparse_tiles(SparseArgs a)
{
	constexpr int RUN = 16 / ES;
	__shared__ unsigned wsum[2][4]; // the waves' counts, two sets in turn: one barrier per trip
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	int set = 0;
	for (int b = blockIdx.y; b < a.batch; b += gridDim.y)
		for (int t = blockIdx.x; t < a.tiles; t += gridDim.x) {
			// the last band whose first tile is not behind t (bands without tiles share their successor's first)
			int lo = 0, hi = a.bands - 1;
			while (lo < hi) {
				const int mid = (lo + hi + 1) >> 1;
				if (a.first[mid] <= t)
					lo = mid;
				else
					hi = mid - 1;
			}
			const int k = lo, w = a.w[k], x0 = a.x0[k], y0 = a.y0[k];
			// samples s .. e of the band's raster order: rows ys .. ye, from column cs of the first to column ce of the last
			const int s = (t - a.first[k]) * SPARSE_TILE_SAMPLES;
			const int e = (int)min((long)s + SPARSE_TILE_SAMPLES, (long)w * a.h[k]) - 1; // (the band's last tile may be shorter)
			const int ys = s / w, cs = s - ys * w, ye = e / w, ce = e - ye * w;
			const int c0 = x0 / RUN, cpr = (x0 + w - 1) / RUN - c0 + 1; // the chunks a band row touches
			const int v_end = (ye - ys + 1) * cpr;
			const char *const frame = a.planes + (long)b * a.bs;
			const unsigned base = PACK ? a.tile[(long)b * a.tiles + t] : 0u;
			unsigned sofar = 0; // PACK: the entries of the trips before; else: this lane's count
			for (int v0 = 0; v0 < v_end; v0 += 256) {
				const int v = v0 + (int)threadIdx.x;
				unsigned bits[RUN];
				unsigned keep = 0; // bit i: sample i of the chunk is the tile's and is kept
				int X0 = 0, y = 0;
#pragma unroll
				for (int i = 0; i < RUN; i++)
					bits[i] = 0;
				if (v < v_end) {
					const int r = v / cpr;
					y = ys + r;
					X0 = (c0 + (v - r * cpr)) * RUN;
					const int lo_x = max(X0, x0 + (r == 0 ? cs : 0)), hi_x = min(X0 + RUN, x0 + (y == ye ? ce + 1 : w));
					if (lo_x < hi_x) {
						const char *const p = frame + (long)(y0 + y) * a.pitch + (long)X0 * ES;
						if (a.wide && X0 + RUN <= a.W) {
							run_load<ES>(p, bits); // (the chunk lies inside the row: own elements of the frame, aligned)
						} else {
#pragma unroll
							for (int i = 0; i < RUN; i++)
								if (X0 + i >= lo_x && X0 + i < hi_x)
									bits[i] = elem_load<ES>(p + i * ES);
						}
#pragma unroll
						for (int i = 0; i < RUN; i++)
							keep |= (unsigned)(X0 + i >= lo_x && X0 + i < hi_x && (bits[i] & a.keep_mask) != 0) << i;
					}
				}
				if constexpr (!PACK) {
					sofar += __popc(keep);
				} else {
					unsigned before = 0, mine = 0; // kept samples of the wave's lower lanes; of the whole wave
#pragma unroll
					for (int i = 0; i < RUN; i++) {
						const unsigned long long m = __ballot((keep >> i) & 1u);
						before += __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
						mine += (unsigned)__popcll(m);
					}
					if (lane == 0)
						wsum[set][wave] = mine;
					__syncthreads();
					unsigned below = 0, all = 0;
#pragma unroll
					for (int q = 0; q < 4; q++) {
						const unsigned c = wsum[set][q];
						below += q < wave ? c : 0u;
						all += c;
					}
					set ^= 1;
					unsigned long long at = (unsigned long long)base + sofar + below + before;
					const unsigned long long out = (unsigned long long)b * a.stream_stride;
					const unsigned p0 = (unsigned)(y0 + y) * (unsigned)a.W + (unsigned)X0;
#pragma unroll
					for (int i = 0; i < RUN; i++)
						if ((keep >> i) & 1u) {
							if (at < a.stream_stride) {
								a.pos[out + at] = p0 + i;
								elem_store<ES>(a.val + (out + at) * ES, bits[i]);
							}
							at++;
						}
					sofar += all;
				}
			}
			if constexpr (!PACK) {
#pragma unroll
				for (int o = 32; o; o >>= 1)
					sofar += __shfl_xor(sofar, o);
				if (lane == 0)
					wsum[set][wave] = sofar;
				__syncthreads();
				if (threadIdx.x == 0)
					a.tile[(long)b * a.tiles + t] = wsum[set][0] + wsum[set][1] + wsum[set][2] + wsum[set][3];
				set ^= 1;
			}
		}
}

constexpr int SCAN_ITEMS = 8; // consecutive tiles of a thread per trip

__global__ __launch_bounds__(256) void k_sparse_scan(SparseArgs a)
{
	__shared__ unsigned wsum[4];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for (int b = blockIdx.x; b < a.batch; b += gridDim.x) {
		unsigned *const tb = a.tile + (long)b * a.tiles;
		unsigned carry = 0;
		for (int t0 = 0; t0 < a.tiles; t0 += 256 * SCAN_ITEMS) {
			const int i0 = t0 + (int)threadIdx.x * SCAN_ITEMS;
			unsigned c[SCAN_ITEMS], sum = 0;
#pragma unroll
			for (int i = 0; i < SCAN_ITEMS; i++) {
				c[i] = i0 + i < a.tiles ? tb[i0 + i] : 0u;
				sum += c[i];
			}
			unsigned incl = sum; // inclusive over the wave's lanes
#pragma unroll
			for (int o = 1; o < 64; o <<= 1) {
				const unsigned up = __shfl_up(incl, o);
				incl += lane >= o ? up : 0u;
			}
			if (lane == 63)
				wsum[wave] = incl;
			__syncthreads();
			unsigned below = 0, all = 0;
#pragma unroll
			for (int q = 0; q < 4; q++) {
				below += q < wave ? wsum[q] : 0u;
				all += wsum[q];
			}
			unsigned at = carry + below + incl - sum;
#pragma unroll
			for (int i = 0; i < SCAN_ITEMS; i++)
				if (i0 + i < a.tiles) {
					tb[i0 + i] = at;
					at += c[i];
				}
			carry += all;
			__syncthreads(); // (wsum is written again; after the last trip: the bases are read below)
		}
		unsigned *const off = a.offsets + (long)b * (a.bands + 1);
		for (int k = threadIdx.x; k <= a.bands; k += 256)
			off[k] = k < a.bands && a.first[k] < a.tiles ? tb[a.first[k]] : carry;
	}
}

template <int ES>
__global__ __launch_bounds__(256) void k_sparse_zero(SparseUnpackArgs a)
{
	constexpr int RUN = 16 / ES;
	const int wave = threadIdx.x >> 6;
	const long x0 = ((long)blockIdx.x * 64 + (threadIdx.x & 63)) * RUN;
	if (x0 >= a.W)
		return;
	const int n = (int)min((long)RUN, a.W - x0);
	const bool wide = a.wide && n == RUN;
	for (int b = blockIdx.z; b < a.batch; b += gridDim.z)
		for (int y = blockIdx.y * 4 + wave; y < a.H; y += gridDim.y * 4) {
			char *const p = a.planes + (long)b * a.bs + (long)y * a.pitch + x0 * ES;
			if (wide) {
				const u4 z = {0u, 0u, 0u, 0u};
				if (a.nt)
					__builtin_nontemporal_store(z, (u4 *)p);
				else
					*(u4 *)p = z;
			} else {
#pragma unroll
				for (int i = 0; i < RUN; i++)
					if (i < n)
						elem_store<ES>(p + i * ES, 0u);
			}
		}
}

template <int ES>
__global__ __launch_bounds__(256) void k_sparse_scatter(SparseUnpackArgs a)
{
	const unsigned samples = (unsigned)a.W * (unsigned)a.H; // (at most INT_MAX)
	for (int b = blockIdx.y; b < a.batch; b += gridDim.y) {
		const unsigned long long n = min((unsigned long long)a.counts[(long)b * a.counts_stride], a.stream_stride);
		const unsigned long long in = (unsigned long long)b * a.stream_stride;
		char *const frame = a.planes + (long)b * a.bs;
		for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
			const unsigned p = a.pos[in + i];
			if (p >= samples)
				continue; // (a foreign stream: never written)
			const unsigned y = p / (unsigned)a.W, x = p - y * (unsigned)a.W;
			elem_store<ES>(frame + (long)y * a.pitch + (long)x * ES, elem_load<ES>(a.val + (in + i) * ES));
		}
	}
}

bool frames_ok(int es, int batch, int W, int H) { return (es == 2 || es == 4) && batch >= 1 && W >= 1 && H >= 1 && (long)W * H <= 2147483647l; }

} // namespace

hipError_t launch_sparse_tiles(int es, bool pack, const SparseArgs &a, hipStream_t s)
{
	if (!frames_ok(es, a.batch, a.W, a.H) || a.bands < 1 || a.bands > BAND_MAX_SLOTS || a.tiles < 1 || a.first[a.bands] != a.tiles || !a.tile ||
	    (pack && (!a.pos || !a.val)))
		return hipErrorInvalidValue;
	// tiles and frames past the caps are taken by the kernel's own loops (tests/test_hip_sparse.py)
	const dim3 grid((unsigned)std::min(a.tiles, SPARSE_GRID_TILES), (unsigned)std::min(a.batch, SPARSE_GRID_BATCH));
	if (es == 2)
		pack ? k_sparse_tiles<2, true><<<grid, 256, 0, s>>>(a) : k_sparse_tiles<2, false><<<grid, 256, 0, s>>>(a);
	else
		pack ? k_sparse_tiles<4, true><<<grid, 256, 0, s>>>(a) : k_sparse_tiles<4, false><<<grid, 256, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_sparse_scan(const SparseArgs &a, hipStream_t s)
{
	if (a.batch < 1 || a.bands < 1 || a.bands > BAND_MAX_SLOTS || a.tiles < 1 || a.first[a.bands] != a.tiles || !a.tile || !a.offsets)
		return hipErrorInvalidValue;
	k_sparse_scan<<<(unsigned)std::min(a.batch, SPARSE_GRID_BATCH), 256, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_sparse_zero(int es, const SparseUnpackArgs &a, hipStream_t s)
{
	if (!frames_ok(es, a.batch, a.W, a.H) || !a.planes)
		return hipErrorInvalidValue;
	const long span = 64l * (16 / es);
	const dim3 grid((unsigned)((a.W + span - 1) / span), (unsigned)std::min<long>(((long)a.H + 3) / 4, SPARSE_GRID_TILES),
		(unsigned)std::min(a.batch, SPARSE_GRID_BATCH));
	if (es == 2)
		k_sparse_zero<2><<<grid, 256, 0, s>>>(a);
	else
		k_sparse_zero<4><<<grid, 256, 0, s>>>(a);
	return hipGetLastError();
}

hipError_t launch_sparse_scatter(int es, const SparseUnpackArgs &a, hipStream_t s)
{
	if (!frames_ok(es, a.batch, a.W, a.H) || !a.planes || !a.pos || !a.val || !a.counts)
		return hipErrorInvalidValue;
	const unsigned long long groups = (a.stream_stride + 255) / 256;
	const dim3 grid((unsigned)std::max<unsigned long long>(1, std::min<unsigned long long>(groups, SPARSE_GRID_TILES)),
		(unsigned)std::min(a.batch, SPARSE_GRID_BATCH));
	if (es == 2)
		k_sparse_scatter<2><<<grid, 256, 0, s>>>(a);
	else
		k_sparse_scatter<4><<<grid, 256, 0, s>>>(a);
	return hipGetLastError();
}

} // namespace dwt
