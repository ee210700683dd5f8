// The decoders' first-maximum rule, ONE definition for every kernel that picks a vocabulary entry (greedy, the pipelined decoder,
// the attention decoders, top-k for beam search, sampling): value descending, and among equal values the LOWEST index wins --
// torch.max(1) and argsort(p)[-k:] of the reference.  Device-only; every merge below is a step of the same total order, so
// which lanes merge in which sequence never changes the winner.
#pragma once
#include "common.h"

constexpr int kNoIndex = 0x7fffffff;   // "no element yet": ranks after every real index of an equal value

// a ranks before b: value descending, index ascending
__device__ __forceinline__ bool ranks_before(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }

// first element of the wave, in every lane
__device__ __forceinline__ void wave_first(float& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64); const int oi = __shfl_xor(i, o, 64);
    if (ranks_before(ov, oi, v, i)) { v = ov; i = oi; }
  }
}

// first element across the wave's four 16-lane groups (lanes r, r + 16, r + 32, r + 48: the four MFMA output quads of one row)
__device__ __forceinline__ void quad_first(float& v, int& i) {
#pragma unroll
  for (int o = 16; o < 64; o <<= 1) {
    const float ov = __shfl_xor(v, o, 64); const int oi = __shfl_xor(i, o, 64);
    if (ranks_before(ov, oi, v, i)) { v = ov; i = oi; }
  }
}

// first element of a 256-thread block, in every thread; sv / si hold 4 entries and may be reused by the next call (leading barrier)
__device__ __forceinline__ void block_first(float& v, int& i, float* sv, int* si) {
  wave_first(v, i);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = v; si[threadIdx.x >> 6] = i; }
  __syncthreads();
  v = sv[0]; i = si[0];
  for (int w = 1; w < 4; ++w) if (ranks_before(sv[w], si[w], v, i)) { v = sv[w]; i = si[w]; }
}

// The same order as ONE unsigned 64-bit number, for atomicMax: the sign-flipped float above, 0xffffffff - index below.  0 means
// "nothing" (a real key has a non-zero index half).  The key order puts +0.0 above -0.0, which the float comparison calls equal.
__device__ __forceinline__ unsigned long long argmax_key(float v, int i) {
  if (i == kNoIndex) return 0ull;
  unsigned u = __float_as_uint(v);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)u << 32) | (unsigned long long)(0xffffffffu - (unsigned)i);
}

// the index of a key; 0 when it is not in [0, V) (an empty key, a row of NaNs)
__device__ __forceinline__ int key_token(unsigned long long key, int V) {
  const int tok = (int)(0xffffffffu - (unsigned)(key & 0xffffffffull));
  return (tok < 0 || tok >= V) ? 0 : tok;
}
