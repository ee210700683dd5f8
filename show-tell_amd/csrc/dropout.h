// The decoders' dropout mask, ONE definition for every kernel that applies it (st_dropout_rows, the DROP forms of rnn_gemm_kernel and
// rnn_bwd_cell_kernel) and for the host: a pure function of (seed, step, site, packed row, column), no generator state anywhere.
//   words  = Philox4x32-10(counter = (column / 4, packed row, site, step), key = (seed low 32, seed high 32))
//   word e of the four belongs to column 4 * (column / 4) + e
//   keep   iff word >= thr,  thr = (uint32) floor(p * 2^32) formed on the host in double, 0 <= p < 1
//   value  = T(float(x) * scale) when kept, scale = float(1 / (1 - p)) formed on the host; +0 when dropped
// The packed row is the time-major row of st_packed_seq (row(t, b) = step_off[t] + b), so the mask depends on no launch geometry,
// tile shape or route.  Sites: l = the output of recurrent layer l (L - 1: the rows in front of `linear`), kDropSiteInput = the
// layer-0 input rows.  Device and host: tests replicate it bit for bit.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ST_DROP_HD __host__ __device__ __forceinline__
#else
#define ST_DROP_HD inline
#endif

constexpr int kDropSiteInput = 255;
constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u, kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

struct DropWords { uint32_t w[4]; };

ST_DROP_HD DropWords philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)kPhiloxM0 * c0, p1 = (uint64_t)kPhiloxM1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += kPhiloxW0; k1 += kPhiloxW1;
  }
  return DropWords{{c0, c1, c2, c3}};
}

// what a kernel needs of one call's dropout at one probability: by value, 20 bytes
struct DropKey { uint32_t seed_lo, seed_hi, step, thr; float scale; };

// the four words of columns col4 * 4 .. col4 * 4 + 3 of packed row `row` at `site`
ST_DROP_HD DropWords drop_words(const DropKey& k, int site, int row, int col4) {
  return philox4x32_10((uint32_t)col4, (uint32_t)row, (uint32_t)site, k.step, k.seed_lo, k.seed_hi);
}
// the multiplier of one element: scale when kept, 0 when dropped
ST_DROP_HD float drop_mult(const DropKey& k, uint32_t word) { return word >= k.thr ? k.scale : 0.f; }

// host: (thr, scale) of a probability; p outside [0, 1) is the caller's error
inline DropKey drop_key(double p, long seed, int step) {
  DropKey k;
  k.seed_lo = (uint32_t)((uint64_t)seed & 0xffffffffu); k.seed_hi = (uint32_t)((uint64_t)seed >> 32);
  k.step = (uint32_t)step;
  k.thr = (uint32_t)(uint64_t)(p * 4294967296.0);
  k.scale = (float)(1.0 / (1.0 - p));
  return k;
}
