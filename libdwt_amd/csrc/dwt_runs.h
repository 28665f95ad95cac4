// dwt_runs.h -- what the kernels that move a lane's run of consecutive samples by 16-byte accesses share (dwt_pixels.hip,
// dwt_quant.hip): a run of 1-, 2- or 4-byte elements held as dwords, and binary16 <-> binary32.
#pragma once
#include "dwt_device.h"

namespace dwt {

typedef unsigned short hbits;
static __device__ __forceinline__ float widen_h(unsigned bits) { return (float)__builtin_bit_cast(_Float16, (hbits)bits); }
static __device__ __forceinline__ unsigned narrow_h(float v) { return __builtin_bit_cast(hbits, (_Float16)v); }

// element k of a run of ES-byte elements held as dwords (k is a constant after unrolling)
template <int ES>
static __device__ __forceinline__ unsigned run_get(const unsigned *raw, int k)
{
	if constexpr (ES == 1)
		return (raw[k >> 2] >> (8 * (k & 3))) & 0xffu;
	else if constexpr (ES == 2)
		return (raw[k >> 1] >> (16 * (k & 1))) & 0xffffu;
	else
		return raw[k];
}
template <int ES>
static __device__ __forceinline__ void run_put(unsigned *raw, int k, unsigned v)
{
	if constexpr (ES == 1)
		raw[k >> 2] |= (v & 0xffu) << (8 * (k & 3));
	else if constexpr (ES == 2)
		raw[k >> 1] |= (v & 0xffffu) << (16 * (k & 1));
	else
		raw[k] = v;
}

// N elements of ES bytes from / to 16-byte aligned memory, N * ES a multiple of 16
template <int ES, int N>
static __device__ __forceinline__ void run_load(const char *p, unsigned (&e)[N])
{
	constexpr int NQ = N * ES / 16;
	unsigned raw[NQ * 4];
#pragma unroll
	for (int q = 0; q < NQ; q++) {
		const u4 t = __builtin_nontemporal_load((const u4 *)p + q); // (every input is read once)
		raw[4 * q] = t.x, raw[4 * q + 1] = t.y, raw[4 * q + 2] = t.z, raw[4 * q + 3] = t.w;
	}
#pragma unroll
	for (int k = 0; k < N; k++)
		e[k] = run_get<ES>(raw, k);
}
template <int ES, int N>
static __device__ __forceinline__ void run_store(char *p, const unsigned (&e)[N], bool nt)
{
	constexpr int NQ = N * ES / 16;
	unsigned raw[NQ * 4];
#pragma unroll
	for (int q = 0; q < NQ * 4; q++)
		raw[q] = 0;
#pragma unroll
	for (int k = 0; k < N; k++)
		run_put<ES>(raw, k, e[k]);
#pragma unroll
	for (int q = 0; q < NQ; q++) {
		const u4 t = {raw[4 * q], raw[4 * q + 1], raw[4 * q + 2], raw[4 * q + 3]};
		if (nt)
			__builtin_nontemporal_store(t, (u4 *)p + q);
		else
			*((u4 *)p + q) = t;
	}
}

} // namespace dwt
