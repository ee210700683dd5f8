// Caption sampling: one token per row drawn from softmax(logits / temperature), optionally restricted to the top_k largest
// logits, with the token's log-probability (include/showtell_hip.h: st_sample_rows, st_rnn_sample).  The multinomial
// counterpart of the max(1)[1] of rnn.py:52 / rnn_attn.py:141.  No random-number generator lives here: the caller hands
// in one uniform per row and step, so every draw is a deterministic function of (logits, u).
//
// One workgroup per row; thread t owns the CONTIGUOUS index range [t * chunk, (t + 1) * chunk), so that index order is
// (thread, position) order:
//   pass 1  per-thread maximum -> row maximum; with top_k > 0 the k-th largest THREAD maximum T0 is a lower bound of the
//           row's k-th largest element (the idea of softmax_topk_thr_kernel), the elements >= T0 go to a candidate list
//           in LDS and the candidate of rank k - 1 (value descending, index ascending: st_softmax_topk's order) is the
//           last kept element (T, Ti): v is kept iff v > T or (v == T and index <= Ti);
//   pass 2  per-thread sum of exp over the kept elements of its range, block scan of the 256 partial sums;
//   pass 3  the first thread whose inclusive sum exceeds u * sum walks its own range (at most `chunk` elements).
// With top_p < 1 (the NUC form) a nucleus search between passes 1 and 2 moves (T, Ti) to the last element of the shortest
// prefix of that order whose mass reaches top_p (of the top_k set when top_k > 0); passes 2 and 3 then run as they are.
// No lane ever sums a whole row.  Rows of up to 256 x 40 entries (V = 10000) are read ONCE, with all of a thread's loads in
// flight together, and stay in registers between the passes; longer or unaligned rows take the passes over memory.
// A row needs at least one finite entry: with none (all -inf or NaN) the token is 0 and logp is NaN.
#include "decoder_host.h"
#include "select.h"
#include <type_traits>

namespace {

constexpr int kSampleThreads = 256;
constexpr int kSampleCap = 1024;      // candidate list; more elements >= T0 (rows of equal logits): exact selection by rounds

// f(value, index) for every index of [lo, hi) in increasing order; lo is a multiple of 4 (16-byte loads when VEC: the row
// is padded to a multiple of 4 entries, so the last load stays inside the row)
template <bool VEC, typename F>
__device__ __forceinline__ void for_range(const float* __restrict__ l, int lo, int hi, F&& f) {
  for (int j = lo; j < hi; j += 4) {
    float v[4];
    if (VEC) {
      const f32x4 q = *reinterpret_cast<const f32x4*>(l + j);
      v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = j + e < hi ? l[j + e] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) if (j + e < hi) f(v[e], j + e);
  }
}

// A thread's view of its index range [lo, hi) of the row: each(f) calls f(value, index) in increasing index order.
template <bool VEC>
struct RowMem {
  const float* l; int lo, hi;
  __device__ __forceinline__ RowMem(const float* l_, int lo_, int hi_) : l(l_), lo(lo_), hi(hi_) {}
  template <typename F> __device__ __forceinline__ void each(F&& f) const { for_range<VEC>(l, lo, hi, f); }
};
constexpr int kSampleRegs = 40;       // entries per thread of the register-resident form
struct RowReg {
  float rv[kSampleRegs]; int lo, hi;
  __device__ __forceinline__ RowReg(const float* l, int lo_, int hi_) : lo(lo_), hi(hi_) {
#pragma unroll
    for (int j = 0; j < kSampleRegs; j += 4) {         // unconditional address arithmetic, predicated loads: all in flight at once
      f32x4 q = {0.f, 0.f, 0.f, 0.f};
      if (lo + j < hi) q = *reinterpret_cast<const f32x4*>(l + lo + j);
      rv[j] = q[0]; rv[j + 1] = q[1]; rv[j + 2] = q[2]; rv[j + 3] = q[3];
    }
  }
  template <typename F> __device__ __forceinline__ void each(F&& f) const {
#pragma unroll
    for (int j = 0; j < kSampleRegs; ++j) if (lo + j < hi) f(rv[j], lo + j);
  }
};

// The nucleus search's view of a thread's range: above(piv) is the sum, in index order, of the weights wf(value, index) of the
// entries with value > piv.  Over memory the weights are recomputed in every round; the register-resident row computes them
// once and keeps them next to the row.
template <typename Row>
struct RowWeights {
  template <typename WF> __device__ __forceinline__ RowWeights(const Row&, WF&&) {}
  template <typename WF> __device__ __forceinline__ float above(const Row& r, float piv, WF&& wf) const {
    float s = 0.f;
    r.each([&](float v, int i) { if (v > piv) s += wf(v, i); });
    return s;
  }
};
template <>
struct RowWeights<RowReg> {
  float w[kSampleRegs];
  template <typename WF> __device__ __forceinline__ RowWeights(const RowReg& r, WF&& wf) {
#pragma unroll
    for (int j = 0; j < kSampleRegs; ++j) w[j] = r.lo + j < r.hi ? wf(r.rv[j], r.lo + j) : 0.f;
  }
  template <typename WF> __device__ __forceinline__ float above(const RowReg& r, float piv, WF&&) const {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < kSampleRegs; ++j) s += r.rv[j] > piv ? w[j] : 0.f;      // + 0 leaves a sum of weights >= 0 as it is
    return s;
  }
};

// float <-> unsigned, order preserving (the value half of select.h::argmax_key); -0.0 sits one below +0.0, and the search
// compares floats, to which the two are one value
__device__ __forceinline__ unsigned ord_of(float v) { const unsigned b = __float_as_uint(v); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ float ord_value(unsigned o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

// Sum of a float over the wave, in every lane, always in the same order: pairs, quads, eights and sixteens inside each row
// of 16 lanes by DPP (no LDS round trip, which six dependent shuffles would make of every round of the search), then the
// four rows in order.
__device__ __forceinline__ float wave_sum_dpp(float x) {
  auto dpp = [](float v, auto ctrl) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), decltype(ctrl)::value, 0xf, 0xf, false));
  };
  x += dpp(x, std::integral_constant<int, 0xB1>{});          // quad_perm [1, 0, 3, 2]
  x += dpp(x, std::integral_constant<int, 0x4E>{});          // quad_perm [2, 3, 0, 1]
  x += dpp(x, std::integral_constant<int, 0x141>{});         // row_half_mirror
  x += dpp(x, std::integral_constant<int, 0x140>{});         // row_mirror: every lane of a row holds the row's sum
  const int xi = __float_as_int(x);
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(xi, 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(xi, 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(xi, 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(xi, 48));
  return ((r0 + r1) + r2) + r3;
}

// What the MIX form (scheduled sampling, st_sample_mix_rows) takes beyond the draw's arguments: the row's slot takes the draw iff the
// step it feeds is inside the row's caption and its coin fell below p; every other row skips the three passes and keeps the
// teacher's token.  No finished state there: the caption decides a row's length.
struct MixArgs {
  const float* coin; int coin_stride; float p;
  const long* teacher; int teacher_stride; long teacher_col;
  const int* lens; int step;
  long* mixed_out; uint8_t* replaced_out;
};

// NUC: top_p < 1, the nucleus search after pass 1 (never with MIX); without it top_p is not read
template <typename Row, bool MIX = false, bool NUC = false>
__global__ __launch_bounds__(kSampleThreads) void sample_rows_kernel(const float* __restrict__ logits, int ldl, int V, const float* __restrict__ u,
                                                                     int u_stride, float inv_t, int top_k, long end_id, uint8_t* __restrict__ finished,
                                                                     long* __restrict__ ids_out, float* __restrict__ logp_out, int out_stride, int t,
                                                                     long* __restrict__ cur, MixArgs mix, float top_p) {
  static_assert(!(MIX && NUC), "the scheduled-sampling draw has no nucleus");
  __shared__ float s_tm[kSampleThreads];
  __shared__ float c_v[kSampleCap]; __shared__ int c_i[kSampleCap];
  __shared__ float s_max[4], s_sum[4], s_bv[4]; __shared__ int s_bi[4], s_last[4], s_first[4];
  __shared__ int s_cnt, s_Ti, s_tok; __shared__ float s_T;
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const long out = (long)row * out_stride + t;
  if constexpr (MIX) {
    // (block-uniform) strict comparison: p = 0 takes nothing, a NaN coin never
    if (!(mix.step < mix.lens[row] && mix.coin[(long)row * mix.coin_stride] < mix.p)) {
      if (tid == 0) {
        const long tk = mix.teacher[(long)row * mix.teacher_stride + mix.teacher_col];
        mix.mixed_out[out] = tk; cur[row] = tk; mix.replaced_out[out] = 0;
        if (ids_out) ids_out[out] = -1;
        if (logp_out) logp_out[out] = 0.f;
      }
      return;
    }
  } else if (finished[row]) {                                // (block-uniform) <pad> after <end>
    if (tid == 0) { ids_out[out] = 0; logp_out[out] = 0.f; if (cur) cur[row] = 0; }
    return;
  }
  const float* l = logits + (long)row * ldl;
  const int chunk = ((V + kSampleThreads - 1) / kSampleThreads + 3) & ~3;
  const int lo = tid * chunk < V ? tid * chunk : V, hi = lo + chunk < V ? lo + chunk : V;
  const Row row_part(l, lo, hi);

  // ---- pass 1: maximum (and the top_k boundary) ----
  float tm = -INFINITY;
  row_part.each([&](float v, int) { tm = fmaxf(tm, v); });
  float M = wave_max(tm);
  if (lane == 0) s_max[wid] = M;
  s_tm[tid] = tm;
  if (tid == 0) s_cnt = 0;
  __syncthreads();
  M = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
  float T = -INFINITY; int Ti = kNoIndex;                    // top_k == 0 (or V): everything is kept
  if (top_k > 0 && top_k < V) {
    int rank = 0;                                            // of this thread's maximum among the 256 (a total order: one thread per rank)
    for (int o = 0; o < kSampleThreads; ++o) rank += ranks_before(s_tm[o], o, tm, tid) ? 1 : 0;
    if (rank == top_k - 1) s_T = tm;
    __syncthreads();
    const float T0 = s_T;                                    // >= top_k elements are >= T0 (T0 = -inf: all V of them)
    row_part.each([&](float v, int i) {
      if (v >= T0) { const int p = atomicAdd(&s_cnt, 1); if (p < kSampleCap) { c_v[p] = v; c_i[p] = i; } }
    });
    __syncthreads();
    const int n = s_cnt;
    if (n <= kSampleCap) {
      for (int c = tid; c < n; c += kSampleThreads) {
        const float v = c_v[c]; const int i = c_i[c];
        int r = 0;
        for (int o = 0; o < n; ++o) r += ranks_before(c_v[o], c_i[o], v, i) ? 1 : 0;
        if (r == top_k - 1) { s_T = v; s_Ti = i; }
      }
    } else {                                                 // (block-uniform) round j picks the first element after round j-1's
      float pv = INFINITY; int pi = -1;
      for (int j = 0; j < top_k; ++j) {
        float bv = -INFINITY; int bi = kNoIndex;
        row_part.each([&](float v, int i) {
          if (ranks_before(pv, pi, v, i) && ranks_before(v, i, bv, bi)) { bv = v; bi = i; }
        });
        block_first(bv, bi, s_bv, s_bi);
        pv = bv; pi = bi;
      }
      if (tid == 0) { s_T = pv; s_Ti = pi; }
    }
    __syncthreads();
    T = s_T; Ti = s_Ti;
  }
  if constexpr (NUC) {
    // ---- the nucleus: (T, Ti) moves to the last element whose preceding mass is below top_p * (mass of the set so far) ----
    // G(x) = sum of the weights of the eligible elements of value > x, always in the same order (a thread's range in index
    // order, wave_sum_dpp, the four waves): floating-point addition is monotone, so G falls as x rises and the smallest
    // x with G(x) < P is well defined.  It is the value of the last kept element; bisection over the order-preserving integer
    // image of the floats between the lowest eligible value and the maximum finds it in at most 32 rounds of one barrier each.
    __shared__ float s_g[2][4]; __shared__ int s_n[4];
    const float Tk = T; const int Tki = Ti;
    auto elig_w = [&](float v, int i) { return (v > Tk || (v == Tk && i <= Tki)) ? expf((v - M) * inv_t) : 0.f; };
    const RowWeights<Row> rw(row_part, elig_w);
    int par = 0;
    auto G = [&](float piv) {
      float g = wave_sum_dpp(rw.above(row_part, piv, elig_w));
      if (lane == 0) s_g[par][wid] = g;
      __syncthreads();                                       // one barrier a round: the next round writes the other half
      g = ((s_g[par][0] + s_g[par][1]) + s_g[par][2]) + s_g[par][3];
      par ^= 1;
      return g;
    };
    const float P = top_p * G(-INFINITY);                    // -inf entries weigh 0
    unsigned xlo = ord_of(Tk), xhi = ord_of(M);              // G(M) = 0 < P
    float Ghi = 0.f;
    while (xlo < xhi) {                                      // (block-uniform: every thread holds the same sums)
      const unsigned mid = xlo + (xhi - xlo) / 2;
      const float g = G(ord_value(mid));
      if (g < P) { xhi = mid; Ghi = g; } else xlo = mid + 1;
    }
    const float Tn = ord_value(xhi);
    // among the elements equal to Tn, which weigh wT each, the first m are kept: the j-th of them (from 0) has Ghi + j * wT
    // before it, a sequence that rises with j.  An integer scan of the per-thread counts finds the m-th one's index.
    int cnt = 0;
    row_part.each([&](float v, int i) { if (v == Tn && (v > Tk || i <= Tki)) ++cnt; });
    int cinc = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(cinc, o, 64); if (lane >= o) cinc += y; }
    if (lane == 63) s_n[wid] = cinc;
    __syncthreads();
    int cex = cinc - cnt;
    for (int w = 0; w < wid; ++w) cex += s_n[w];
    const int neq = s_n[0] + s_n[1] + s_n[2] + s_n[3];
    const float wT = expf((Tn - M) * inv_t);
    int mlo = 1, mhi = neq;                                  // the largest m in [1, neq] with Ghi + (m - 1) * wT < P; m = 1 holds: Ghi < P
    while (mlo < mhi) {
      const int mm = mlo + (mhi - mlo + 1) / 2;
      if (Ghi + (float)(mm - 1) * wT < P) mlo = mm; else mhi = mm - 1;
    }
    if (cex < mlo && mlo <= cex + cnt) {                     // one thread: the m-th equal element is in its range
      int seen = cex;
      row_part.each([&](float v, int i) { if (v == Tn && (v > Tk || i <= Tki) && ++seen == mlo) { s_T = Tn; s_Ti = i; } });
    }
    __syncthreads();
    if (neq > 0) { T = s_T; Ti = s_Ti; }                     // neq == 0: a row of NaNs, the set stays what it was
  }
  auto kept = [&](float v, int i) { return v > T || (v == T && i <= Ti); };
  // (v - M) * inv_t, not v * inv_t - M * inv_t: exactly 0 at the maximum, and no product feeds an addition that the
  // compiler could contract into a fused multiply-add in one pass and not in the other
  auto weight = [&](float v) { return expf((v - M) * inv_t); };

  // ---- pass 2: partial sums over contiguous ranges, block scan ----
  float loc = 0.f; int lastk = -1;
  row_part.each([&](float v, int i) { if (kept(v, i)) { loc += weight(v); lastk = i; } });
  float inc = loc;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const float y = __shfl_up(inc, o, 64); if (lane >= o) inc += y; }
  float excl = __shfl_up(inc, 1, 64);
  if (lane == 0) excl = 0.f;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) lastk = max(lastk, __shfl_xor(lastk, o, 64));
  if (lane == 63) s_sum[wid] = inc;
  if (lane == 0) s_last[wid] = lastk;
  __syncthreads();
  float woff = 0.f;
  for (int w = 0; w < wid; ++w) woff += s_sum[w];
  excl += woff;
  const float S = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
  const float target = u[(long)row * u_stride] * S;

  // ---- pass 3: the first range that crosses u * S, and a walk inside it ----
  int first = (loc > 0.f && excl + loc > target) ? tid : kSampleThreads;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
  if (lane == 0) s_first[wid] = first;
  __syncthreads();
  first = min(min(s_first[0], s_first[1]), min(s_first[2], s_first[3]));
  if (tid == first) {                                        // the same additions in the same order as pass 2: run ends at loc
    float run = 0.f; int tok = -1;
    row_part.each([&](float v, int i) {
      if (kept(v, i)) { run += weight(v); if (tok < 0 && excl + run > target) tok = i; }
    });
    s_tok = tok;
  } else if (first == kSampleThreads && tid == 0) {          // rounding left no crossing: the largest kept index
    s_tok = max(max(s_last[0], s_last[1]), max(s_last[2], s_last[3]));
  }
  __syncthreads();
  if (tid == 0) {
    int tok = s_tok;
    if (tok < 0 || tok >= V) tok = 0;                        // a row without a finite entry: keep the index in range (logp is NaN)
    if constexpr (MIX) {
      mix.mixed_out[out] = tok; cur[row] = tok; mix.replaced_out[out] = 1;
      if (ids_out) ids_out[out] = tok;
      if (logp_out) logp_out[out] = (l[tok] - M) * inv_t - logf(S);
    } else {
      ids_out[out] = tok;
      logp_out[out] = (l[tok] - M) * inv_t - logf(S);
      if (cur) cur[row] = tok;
      if (tok == end_id) finished[row] = 1;
    }
  }
}

}  // namespace

namespace {
template <typename Row>
void launch_sample_rows(bool nucleus, int n, hipStream_t st, const float* logits, int ldl, int V, const float* u, int u_stride, float inv_t, int top_k,
                        long end_id, uint8_t* finished, long* ids_out, float* logp_out, int out_stride, int t, long* cur, float top_p) {
  if (nucleus)
    hipLaunchKernelGGL((sample_rows_kernel<Row, false, true>), dim3(n), dim3(kSampleThreads), 0, st, logits, ldl, V, u, u_stride, inv_t, top_k, end_id,
                       finished, ids_out, logp_out, out_stride, t, cur, MixArgs{}, top_p);
  else
    hipLaunchKernelGGL(sample_rows_kernel<Row>, dim3(n), dim3(kSampleThreads), 0, st, logits, ldl, V, u, u_stride, inv_t, top_k, end_id, finished,
                       ids_out, logp_out, out_stride, t, cur, MixArgs{}, 1.f);
}
}  // namespace

extern "C" int st_sample_rows(const float* logits, int ldl, int n, int V, const float* u, int u_stride, float inv_temperature, int top_k,
                              long end_id, uint8_t* finished, long* ids_out, float* logp_out, int out_stride, int t, long* cur, void* stream) {
  return st_sample_rows_topp(logits, ldl, n, V, u, u_stride, inv_temperature, top_k, 1.f, end_id, finished, ids_out, logp_out, out_stride, t, cur, stream);
}

extern "C" int st_sample_rows_topp(const float* logits, int ldl, int n, int V, const float* u, int u_stride, float inv_temperature, int top_k,
                                   float top_p, long end_id, uint8_t* finished, long* ids_out, float* logp_out, int out_stride, int t, long* cur,
                                   void* stream) {
  ST_CHECK(top_p > 0.f && top_p <= 1.f, "st_sample_rows: need 0 < top_p <= 1 (got %g)", (double)top_p);      // NaN fails both
  ST_CHECK(logits && u && finished && ids_out && logp_out, "st_sample_rows: null pointer");
  ST_CHECK(V >= 1 && ldl >= V, "st_sample_rows: need 1 <= V <= ldl (got V=%d ldl=%d)", V, ldl);
  ST_CHECK(inv_temperature > 0.f, "st_sample_rows: inv_temperature must be > 0");
  ST_CHECK(top_k >= 0 && top_k <= 32 && top_k <= V, "st_sample_rows: need 0 <= top_k <= min(32, V) (got %d)", top_k);
  ST_CHECK(t >= 0 && t < out_stride && u_stride >= 0, "st_sample_rows: bad output column %d of %d", t, out_stride);
  if (n <= 0) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool vec = ldl % 4 == 0 && reinterpret_cast<uintptr_t>(logits) % 16 == 0;
  const bool regs = vec && V <= kSampleThreads * kSampleRegs;       // the kernel's chunk = V / 256 rounded up to 4 fits kSampleRegs
  const bool nucleus = top_p < 1.f;                                  // top_p = 1 is the feature off: the launch st_sample_rows always made
  if (regs)
    launch_sample_rows<RowReg>(nucleus, n, st, logits, ldl, V, u, u_stride, inv_temperature, top_k, end_id, finished, ids_out, logp_out, out_stride, t, cur, top_p);
  else if (vec)
    launch_sample_rows<RowMem<true>>(nucleus, n, st, logits, ldl, V, u, u_stride, inv_temperature, top_k, end_id, finished, ids_out, logp_out, out_stride, t, cur, top_p);
  else
    launch_sample_rows<RowMem<false>>(nucleus, n, st, logits, ldl, V, u, u_stride, inv_temperature, top_k, end_id, finished, ids_out, logp_out, out_stride, t, cur, top_p);
  ST_LAUNCH_CHECK();
  return 0;
}

extern "C" int st_sample_mix_rows(const float* logits, int ldl, int n, int V, const float* u, int u_stride, float inv_temperature, int top_k,
                                  const float* coin, int coin_stride, float p, const long* teacher, int teacher_stride, long teacher_col,
                                  const int* lens, int step, long* ids_out, float* logp_out, long* mixed_out, uint8_t* replaced_out,
                                  int out_stride, int t, long* cur, void* stream) {
  ST_CHECK(logits && u && coin && teacher && lens && mixed_out && replaced_out && cur, "st_sample_mix_rows: null pointer");
  ST_CHECK(V >= 1 && ldl >= V, "st_sample_mix_rows: need 1 <= V <= ldl (got V=%d ldl=%d)", V, ldl);
  ST_CHECK(inv_temperature > 0.f, "st_sample_mix_rows: inv_temperature must be > 0");
  ST_CHECK(top_k >= 0 && top_k <= 32 && top_k <= V, "st_sample_mix_rows: need 0 <= top_k <= min(32, V) (got %d)", top_k);
  ST_CHECK(p >= 0.f && p <= 1.f, "st_sample_mix_rows: p=%g outside [0, 1]", (double)p);
  ST_CHECK(t >= 0 && t < out_stride && u_stride >= 0 && coin_stride >= 0, "st_sample_mix_rows: bad output column %d of %d", t, out_stride);
  ST_CHECK(teacher_stride >= 0 && teacher_col >= 0 && step >= 0, "st_sample_mix_rows: bad teacher column or step");
  if (n <= 0) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const bool vec = ldl % 4 == 0 && reinterpret_cast<uintptr_t>(logits) % 16 == 0;
  const bool regs = vec && V <= kSampleThreads * kSampleRegs;       // the routes of st_sample_rows
  const MixArgs mix = {coin, coin_stride, p, teacher, teacher_stride, teacher_col, lens, step, mixed_out, replaced_out};
  if (regs)
    hipLaunchKernelGGL((sample_rows_kernel<RowReg, true>), dim3(n), dim3(kSampleThreads), 0, st, logits, ldl, V, u, u_stride, inv_temperature, top_k, 0L,
                       (uint8_t*)nullptr, ids_out, logp_out, out_stride, t, cur, mix, 1.f);
  else if (vec)
    hipLaunchKernelGGL((sample_rows_kernel<RowMem<true>, true>), dim3(n), dim3(kSampleThreads), 0, st, logits, ldl, V, u, u_stride, inv_temperature, top_k,
                       0L, (uint8_t*)nullptr, ids_out, logp_out, out_stride, t, cur, mix, 1.f);
  else
    hipLaunchKernelGGL((sample_rows_kernel<RowMem<false>, true>), dim3(n), dim3(kSampleThreads), 0, st, logits, ldl, V, u, u_stride, inv_temperature, top_k,
                       0L, (uint8_t*)nullptr, ids_out, logp_out, out_stride, t, cur, mix, 1.f);
  ST_LAUNCH_CHECK();
  return 0;
}

// ---- the plain decoders' sampling loop (rnn.py:37-58 with a draw in place of max(1)[1]) --------------------------------------
namespace {
struct SPlan { size_t h[2], c[2], x, logits, cur, fin, total; };
SPlan make_splan(const st_rnn_params* p, int n) {
  const size_t es = st_dtype_size(p->dtype);
  SPlan q; Arena ar;
  const size_t hb = (size_t)p->L * n * p->H * es;
  for (int i = 0; i < 2; ++i) { q.h[i] = ar.take(hb); q.c[i] = ar.take(p->cell == ST_CELL_LSTM ? hb : 0); }
  q.x = ar.take((size_t)n * p->E * es);
  q.logits = ar.take((size_t)n * st_up8(p->V) * sizeof(float));
  q.cur = ar.take((size_t)n * sizeof(long));
  q.fin = ar.take((size_t)n);
  q.total = ar.o;
  return q;
}
}  // namespace

extern "C" size_t st_rnn_sample_workspace_bytes(const st_rnn_params* p, int n) {
  if (!p || n <= 0 || p->L < 1 || p->L > ST_MAX_LAYERS) return 0;
  return make_splan(p, n).total;
}

extern "C" int st_rnn_sample(const st_rnn_params* p, const void* feat, int n, int steps, const float* u, float inv_temperature, int top_k,
                             long end_id, void* workspace, size_t workspace_bytes, long* ids_out, float* logp_out, void* stream) {
  return st_rnn_sample_topp(p, feat, n, steps, u, inv_temperature, top_k, 1.f, end_id, workspace, workspace_bytes, ids_out, logp_out, stream);
}

extern "C" int st_rnn_sample_topp(const st_rnn_params* p, const void* feat, int n, int steps, const float* u, float inv_temperature, int top_k,
                                  float top_p, long end_id, void* workspace, size_t workspace_bytes, long* ids_out, float* logp_out, void* stream) {
  ST_CHECK(top_p > 0.f && top_p <= 1.f, "st_rnn_sample: need 0 < top_p <= 1 (got %g)", (double)top_p);
  ST_CHECK(p && feat && u && workspace && ids_out && logp_out, "st_rnn_sample: null pointer");
  ST_CHECK(n > 0 && steps > 0, "st_rnn_sample: need n > 0 and steps > 0");
  ST_CHECK(p->L >= 1 && p->L <= ST_MAX_LAYERS && p->in0 == p->E, "st_rnn_sample: bad decoder configuration");
  ST_CHECK(p->emb && p->w_lin && p->b_lin, "st_rnn_sample: null weights");
  const SPlan q = make_splan(p, n);
  ST_CHECK(workspace_bytes >= q.total, "st_rnn_sample: workspace too small");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* ws = reinterpret_cast<char*>(workspace);
  const bool lstm = p->cell == ST_CELL_LSTM;
  const int Vp = st_up8(p->V);
  float* logits = reinterpret_cast<float*>(ws + q.logits);
  long* cur = reinterpret_cast<long*>(ws + q.cur);
  uint8_t* fin = reinterpret_cast<uint8_t*>(ws + q.fin);
  if (hipMemsetAsync(fin, 0, (size_t)n, st) != hipSuccess) { st_set_error("st_rnn_sample: memset failed"); return 1; }
  int c = 0;
  for (int t = 0; t < steps; ++t) {
    const int nx = c ^ 1;
    // step 0: the image feature from a zero state (rnn.py:44-47); later steps: the embedding of the row's last token (rnn.py:53)
    if (st_rnn_step(p, t == 0 ? feat : ws + q.x, n, t == 0 ? nullptr : ws + q.h[c], (t == 0 || !lstm) ? nullptr : ws + q.c[c], ws + q.h[nx],
                    lstm ? ws + q.c[nx] : nullptr, logits, Vp, stream)) return 1;
    if (st_sample_rows_topp(logits, Vp, n, p->V, u + t, steps, inv_temperature, top_k, top_p, end_id, fin, ids_out, logp_out, steps, t, cur, stream)) return 1;
    if (t + 1 < steps && st_embedding_rows(p->emb, cur, ws + q.x, n, p->E, p->V, p->E, p->dtype, stream)) return 1;
    c = nx;
  }
  return 0;
}

// ---- scheduled sampling: the roll-in of the plain decoders (the loop above, following the caption instead of free-running) ----
extern "C" size_t st_rnn_sched_inputs_workspace_bytes(const st_rnn_params* p, int n) { return st_rnn_sample_workspace_bytes(p, n); }

extern "C" int st_rnn_sched_inputs(const st_rnn_params* p, const void* feat, int n, const long* caption, int Tcap, const int* lens, int max_len,
                                   const float* coin, const float* u, float prob, float inv_temperature, int top_k, void* workspace,
                                   size_t workspace_bytes, long* input_ids, uint8_t* replaced, long* drawn, float* logp, void* stream) {
  ST_CHECK(p && feat && caption && lens && coin && u && workspace && input_ids && replaced, "st_rnn_sched_inputs: null pointer");
  ST_CHECK(n > 0 && max_len >= 1 && max_len <= Tcap, "st_rnn_sched_inputs: need n > 0 and 1 <= max_len <= Tcap (got %d, %d)", max_len, Tcap);
  ST_CHECK(p->L >= 1 && p->L <= ST_MAX_LAYERS && p->in0 == p->E, "st_rnn_sched_inputs: bad decoder configuration");
  ST_CHECK(p->emb && p->w_lin && p->b_lin, "st_rnn_sched_inputs: null weights");
  const SPlan q = make_splan(p, n);
  ST_CHECK(workspace_bytes >= q.total, "st_rnn_sched_inputs: workspace too small");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* ws = reinterpret_cast<char*>(workspace);
  const bool lstm = p->cell == ST_CELL_LSTM;
  const int Vp = st_up8(p->V);
  float* logits = reinterpret_cast<float*>(ws + q.logits);
  long* cur = reinterpret_cast<long*>(ws + q.cur);
  if (st_sched_init_outputs(caption, n, Tcap, input_ids, replaced, drawn, logp, st, "st_rnn_sched_inputs")) return 1;
  int c = 0;
  for (int t = 0; t + 1 < max_len; ++t) {           // step t's logits decide slot t, which feeds step t + 1; the last step's are never fed
    const int nx = c ^ 1;
    if (st_rnn_step(p, t == 0 ? feat : ws + q.x, n, t == 0 ? nullptr : ws + q.h[c], (t == 0 || !lstm) ? nullptr : ws + q.c[c], ws + q.h[nx],
                    lstm ? ws + q.c[nx] : nullptr, logits, Vp, stream)) return 1;
    if (st_sample_mix_rows(logits, Vp, n, p->V, u + t, Tcap, inv_temperature, top_k, coin + t, Tcap, prob, caption, Tcap, t, lens, t + 1, drawn,
                           logp, input_ids, replaced, Tcap, t, cur, stream)) return 1;
    if (t + 2 < max_len && st_embedding_rows(p->emb, cur, ws + q.x, n, p->E, p->V, p->E, p->dtype, stream)) return 1;
    c = nx;
  }
  return 0;
}
