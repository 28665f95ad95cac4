// dwt_codeblock_read.h -- what the kernels that measure code-blocks share (k_codeblock_bitplanes of dwt_quant.hip, the
// size launch of dwt_bitplane.hip): which band a block of a prefix table lies in, and the largest magnitude of a block's
// samples, read by one wave -- by whole 16-byte chunks where the frames' rows are 16-byte aligned, element by element
// elsewhere.  The index planes are read once, non-temporally on the 16-byte route.
#pragma once
#include "dwt_device.h"
#include "dwt_runs.h"

namespace dwt {

// the last band whose first block is not behind t (bands without blocks share their successor's first)
static __device__ __forceinline__ int codeblock_band(const int *first, int nbands, int t)
{
	int lo = 0, hi = nbands - 1;
	while (lo < hi) {
		const int mid = (lo + hi + 1) >> 1;
		if (first[mid] <= t)
			lo = mid;
		else
			hi = mid - 1;
	}
	return lo;
}

// The largest |q| of the cw x ch samples from p on (rows `pitch` bytes apart), in every lane of the wave.  `lead_bytes`:
// the byte offset of the block's first column in its row, whose low four bits place the block within its 16-byte chunk.
template <int INDEX>
static __device__ __forceinline__ unsigned codeblock_max_magnitude(const char *p, long pitch, long lead_bytes, int cw, int ch, int cbx, int wide,
	int lane)
{
	constexpr int ES = quant_index_es(INDEX);
	unsigned mx = 0;
	if (wide) {
		// Rows start on 16-byte boundaries and span a multiple of 16 bytes (the driver asked base, pitch and batch stride):
		// the block's bytes of a row, widened to whole 16-byte chunks, stay inside the row's span.  A lane takes a chunk
		// and leaves out the elements in front of and behind the block.
		const long lead = lead_bytes & 15; // the block's first byte within its chunk
		const int chunks = (int)((lead + (long)cw * ES + 15) >> 4);
		const int span = cw * ES;
		for (int i = lane; i < ch * chunks; i += 64) {
			const int y = i / chunks, c = i - y * chunks;
			const long off = ((long)c << 4) - lead; // of the chunk's first byte from the block's first byte of the row
			const u4 t = __builtin_nontemporal_load((const u4 *)(p + (long)y * pitch + off));
			const unsigned raw[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
			for (int e = 0; e < 16 / ES; e++) {
				const long at = off + e * ES;
				const int q = INDEX == kIndexI16 ? (int)(short)run_get<ES>(raw, e) : (int)raw[e];
				const unsigned mag = q < 0 ? 0u - (unsigned)q : (unsigned)q;
				mx = at >= 0 && at < span ? max(mx, mag) : mx;
			}
		}
	} else {
		const int cells = ch << cbx; // the rows of the block at its full width: a cell past a partial block's edge is skipped
#pragma unroll 4
		for (int i = lane; i < cells; i += 64) {
			const int x = i & ((1 << cbx) - 1), y = i >> cbx;
			if (x < cw) {
				unsigned bits;
				if constexpr (ES == 2)
					bits = *(const unsigned short *)(p + (long)y * pitch + (long)x * ES);
				else
					bits = *(const unsigned *)(p + (long)y * pitch + (long)x * ES);
				const int q = INDEX == kIndexI16 ? (int)(short)bits : (int)bits;
				mx = max(mx, q < 0 ? 0u - (unsigned)q : (unsigned)q);
			}
		}
	}
#pragma unroll
	for (int o = 32; o; o >>= 1)
		mx = max(mx, __shfl_xor(mx, o));
	return mx;
}

} // namespace dwt
