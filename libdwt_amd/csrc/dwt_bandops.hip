// dwt_bandops.hip -- the kernel of the per-band coefficient operators: what the reference's synthesis
// programs do between a forward and an inverse transform -- dwt_util_scale_s and dwt_util_compress_s on a subband
// (examples/hdr/hdr.c), zeroing of subbands (examples/mra/mra.c, examples/displ-vectors/vectors.c), the shrinkage behind
// src/denoise.c -- and the two pointwise maps of the hdr flow (logf(c + eps), expf(c) - eps), on coefficients that stay
// where they lie.
//
// ONE launch covers every slot of every image of a batch.  A slot's band is cut into chunks of about BAND_CHUNK
// elements; workgroup g takes chunk g % chunks of image g / chunks and finds its slot in the prefix table of the slots'
// chunk counts, which arrives with the slot geometry and the operator table as kernel arguments (uniform per workgroup:
// scalar loads, no device buffer).  A 4 x 4 LL and a 4096 x 4096 HH share the launch without idle workgroups; slots
// that no image touches have no chunks at all.
//
// A band starts ceil(size / 2^j) elements into a row, so neither its rows nor the pitch are 16-byte aligned in general:
// per row the lanes peel the elements in front of the first 16-byte boundary and behind the last one and take the rest
// as aligned 16-byte accesses.  A band narrower than one vector is all peel.  No byte outside a band is read or written,
// a KEEP slot is neither read nor written, a ZERO slot is written only.
//
// Numerics: SCALE, HARD and SOFT are float arithmetic as written; COMPRESS, LOG and EXP evaluate pow / log / exp in double
// and round to float once (within 1 ulp of the correctly rounded float; the reference calls powf / logf / expf).  A NaN
// coefficient is left as it is by every operator but ZERO.
#include "dwt_device.h"
#include "dwt_kernels.h"

namespace dwt {

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

#include "dwt_band_op.h"

// `rows` rows of `w` elements from `p` on, `pitch` bytes apart: a power of two of lanes along a row, the others on
// further rows
template <int OP>
static __device__ __forceinline__ void walk_rows(char *p, long pitch, int w, int rows, float a)
{
	constexpr bool kReads = OP != kBandZero;
	const int q = (w + 3) >> 2;
	int lg = 0;
	while (lg < 8 && (1 << lg) < q)
		lg++;
	const int TX = 1 << lg, TY = 256 >> lg, tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> lg;
	for (int r = ty; r < rows; r += TY) {
		float *row = (float *)(p + (long)r * pitch);
		const int lead = (int)(((16 - ((uintptr_t)row & 15)) & 15) >> 2); // elements in front of the first 16-byte boundary
		const int head = lead < w ? lead : w, nv = (w - head) >> 2, tail = head + 4 * nv;
		for (int e = tx; e < head; e += TX)
			row[e] = band_op<OP>(kReads ? row[e] : 0.f, a);
		f4 *v = (f4 *)(row + head);
		for (int i = tx; i < nv; i += TX) {
			f4 x = kReads ? v[i] : f4{0.f, 0.f, 0.f, 0.f};
			x.x = band_op<OP>(x.x, a);
			x.y = band_op<OP>(x.y, a);
			x.z = band_op<OP>(x.z, a);
			x.w = band_op<OP>(x.w, a);
			v[i] = x;
		}
		for (int e = tail + tx; e < w; e += TX)
			row[e] = band_op<OP>(kReads ? row[e] : 0.f, a);
	}
}

__global__ __launch_bounds__(256) void k_band_ops(BandOpsArgs a)
{
	const int chunks = a.first[a.nslots];
	const long total = (long)a.batch * chunks;
	for (long g = blockIdx.x; g < total; g += gridDim.x) {
		const long b = g / chunks;
		const int ci = (int)(g % chunks);
		// the last slot whose first chunk is not behind ci (slots without chunks share their successor's first)
		int lo = 0, hi = a.nslots - 1;
		while (lo < hi) {
			const int mid = (lo + hi + 1) >> 1;
			if (a.first[mid] <= ci)
				lo = mid;
			else
				hi = mid - 1;
		}
		const int k = lo;
		const int op = a.dev_op ? a.dev_op[b * a.tstride + k] : (int)a.op[k];
		if (op == kBandKeep)
			continue;
		const float prm = a.dev_param ? a.dev_param[b * a.tstride + k] : a.param[k];
		const int w = a.w[k], h = a.h[k], cw = band_chunk_cols(w), rh = band_chunk_rows(w);
		const int ncc = (w + cw - 1) / cw, ls = ci - a.first[k], cc = ls % ncc, rc = ls / ncc;
		const int c0 = cc * cw, cn = min(cw, w - c0), r0 = rc * rh, rows = min(rh, h - r0);
		char *p = a.img + b * a.bstride + (long)(a.y0[k] + r0) * a.pitch + 4l * (a.x0[k] + c0);
		switch (op) {
		case kBandZero:
			walk_rows<kBandZero>(p, a.pitch, cn, rows, prm);
			break;
		case kBandScale:
			walk_rows<kBandScale>(p, a.pitch, cn, rows, prm);
			break;
		case kBandHard:
			walk_rows<kBandHard>(p, a.pitch, cn, rows, prm);
			break;
		case kBandSoft:
			walk_rows<kBandSoft>(p, a.pitch, cn, rows, prm);
			break;
		case kBandCompress:
			walk_rows<kBandCompress>(p, a.pitch, cn, rows, prm);
			break;
		case kMapLog:
			walk_rows<kMapLog>(p, a.pitch, cn, rows, prm);
			break;
		case kMapExp:
			walk_rows<kMapExp>(p, a.pitch, cn, rows, prm);
			break;
		}
	}
}

} // namespace

hipError_t launch_band_ops(const BandOpsArgs &a, hipStream_t s)
{
	if (a.nslots < 1 || a.nslots > BAND_MAX_SLOTS || a.batch < 0)
		return hipErrorInvalidValue;
	const long total = (long)a.batch * a.first[a.nslots];
	if (total <= 0)
		return hipSuccess;
	const long cap = 256 * 64; // 64 workgroups on each of the 256 CUs, the rest by the grid-stride loop (past the cap: tests/test_hip_grid_limits.py)
	k_band_ops<<<(unsigned)(total < cap ? total : cap), 256, 0, s>>>(a);
	return hipGetLastError();
}

} // namespace dwt
