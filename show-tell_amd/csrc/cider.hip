// CIDEr rewards of sampled captions on the device (st_cider_reward): the score of evaluation.cider_score, restated over packed
// 64-bit n-gram keys and a sorted (key, document frequency) table, one workgroup per image, everything else in LDS.
//
//   phase A  the image's references: every (reference, order, position) item packs its n-gram, counts tf by comparing the keys
//            of the same reference and order position by position, finds df by binary search in the global table (a miss is
//            df = 0, i.e. idf = log N) and leaves (key, weight, first-occurrence flag) in LDS; one thread per (reference, order)
//            then adds the squared weights of the first occurrences in position order.
//   phase B  one wave per candidate in turn (the S samples, then the greedy caption; eight waves, so S = 5 and the greedy caption
//            take one round): lane i owns position i and its four n-grams.  The candidate never leaves registers -- a lane sees
//            the other positions' keys by reading their lanes -- and is contracted against every reference by scanning that
//            reference's keys of the same order (every lane reads the same LDS address: a broadcast).
//   baseline after a barrier, one thread per sample, from the float32 rewards the block has just written.
//
// All arithmetic is float64 on the VALU.  Every sum runs in a fixed order (position order, or the xor tree of wave_sum_f64), so a
// call is a pure function of its inputs: two identical captions get bit-identical scores whatever their padding.
#include "common.h"
#include <math.h>

namespace {

constexpr int kMaxRefs = ST_CIDER_MAX_REFS;      // 8
constexpr int kMaxLen = ST_CIDER_MAX_TOKENS;     // 64: one wave lane per position
constexpr int kOrders = 4;
constexpr int kThreads = 512;                   // 8 waves: phase B scores 5 samples and the greedy caption in one round
constexpr int kWaves = kThreads / 64;
constexpr int kItems = kMaxRefs * kOrders * kMaxLen / kThreads;     // phase A items per thread (4)

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// lane l's copy of v, l wave-uniform: two scalar lane reads, where a shuffle would go through the LDS crossbar
__device__ __forceinline__ uint64_t lane_read(uint64_t v, int l) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
  return (uint64_t)hi << 32 | lo;
}

// token field of position j of an n-gram: (id + 1) << (16 * j); ids are in [0, 65534], so a field is never 0 and the highest
// non-zero field gives the order
__device__ __forceinline__ uint64_t field(int id) { return (uint64_t)(uint32_t)(id + 1) & 0xffffu; }

// Document frequencies of NQ keys at once: NQ independent lower-bound searches in step with each other, so that each round has NQ
// loads in flight instead of one (the searches are chains of ~log2 K dependent loads).  The table is sorted as SIGNED int64.
template <int NQ>
__device__ __forceinline__ void table_df(const long* __restrict__ keys, const int* __restrict__ df, long K, const uint64_t (&q)[NQ],
                                         const bool (&valid)[NQ], int (&out)[NQ]) {
  long base[NQ];
#pragma unroll
  for (int a = 0; a < NQ; ++a) { base[a] = 0; out[a] = 0; }
  if (K <= 0) return;
  for (long len = K; len > 1;) {
    const long half = len >> 1;
#pragma unroll
    for (int a = 0; a < NQ; ++a) {
      const long probe = valid[a] ? keys[base[a] + half - 1] : 0;
      base[a] += (valid[a] && probe < (long)q[a]) ? half : 0;
    }
    len -= half;
  }
#pragma unroll
  for (int a = 0; a < NQ; ++a)
    if (valid[a] && keys[base[a]] == (long)q[a]) out[a] = df[base[a]];
}

__device__ __forceinline__ double tfidf(int tf, int df, double log_docs) {
  return (double)tf * (log_docs - log((double)(df > 1 ? df : 1)));
}

struct Shared {
  uint64_t key[kMaxRefs][kOrders][kMaxLen];      // 0 where the reference has no n-gram at that position
  double w[kMaxRefs][kOrders][kMaxLen];          // the n-gram's weight, the same at each of its occurrences
  uint8_t first[kMaxRefs][kOrders][kMaxLen];     // 1 at an n-gram's first occurrence
  double norm[kMaxRefs][kOrders];
  int tok[kMaxRefs][kMaxLen + kOrders];          // token fields, 0 past the reference's words
  int words[kMaxRefs];
};

__global__ __launch_bounds__(kThreads) void cider_reward_kernel(
    const long* __restrict__ tkeys, const int* __restrict__ tdf, long K, double log_docs, const int* __restrict__ refs,
    const int* __restrict__ ref_len, const int* __restrict__ ref_count, int R, int Tr, const long* __restrict__ ids,
    const long* __restrict__ lengths, int S, int T, const long* __restrict__ greedy_ids, int Tg, long end_id, double inv_two_sigma2,
    int baseline, double* __restrict__ score64, float* reward, float* __restrict__ advantage) {
  __shared__ Shared sh;
  __shared__ float greedy_reward;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int nref = ref_count[b];
  nref = nref < 0 ? 0 : nref > R ? R : nref;

  // ---- phase A: the references ------------------------------------------------------------------------------------------
  for (int i = tid; i < kMaxRefs * (kMaxLen + kOrders); i += kThreads) {
    const int r = i / (kMaxLen + kOrders), j = i % (kMaxLen + kOrders);
    int words = 0;
    if (r < nref) { words = ref_len[(long)b * R + r]; words = words < 0 ? 0 : words > Tr ? Tr : words; }
    sh.tok[r][j] = j < words ? (int)field(refs[((long)b * R + r) * Tr + j]) : 0;
    if (j == 0) sh.words[r] = words;
  }
  __syncthreads();
  uint64_t key[kItems];
  bool valid[kItems];
#pragma unroll
  for (int a = 0; a < kItems; ++a) {               // item (r, n, j): the wave owns an order and every kWaves / 4-th reference, the lane a position
    const int r = a * (kWaves / kOrders) + wave / kOrders, n = wave % kOrders, j = lane;
    valid[a] = j + n + 1 <= sh.words[r];
    uint64_t k = 0;
    for (int m = 0; m <= n; ++m) k |= (uint64_t)sh.tok[r][j + m] << (16 * m);
    key[a] = valid[a] ? k : 0;
    sh.key[r][n][j] = key[a];
  }
  __syncthreads();
  int df[kItems];
  table_df<kItems>(tkeys, tdf, K, key, valid, df);
#pragma unroll
  for (int a = 0; a < kItems; ++a) {
    const int r = a * (kWaves / kOrders) + wave / kOrders, n = wave % kOrders, j = lane;
    const int npos = sh.words[r] - n;              // positions of this reference that hold an n-gram of this order
    int tf = 0, before = 0;
    for (int m = 0; m < npos; ++m) {
      const int same = sh.key[r][n][m] == key[a];
      tf += same;
      before += same & (m < j);
    }
    sh.w[r][n][j] = valid[a] ? tfidf(tf, df[a], log_docs) : 0.0;
    sh.first[r][n][j] = valid[a] && before == 0;
  }
  __syncthreads();
  if (tid < kMaxRefs * kOrders) {
    const int r = tid / kOrders, n = tid % kOrders;
    double acc = 0.0;
    for (int m = 0; m < sh.words[r] - n; ++m)
      if (sh.first[r][n][m]) acc += sh.w[r][n][m] * sh.w[r][n][m];
    sh.norm[r][n] = sqrt(acc);
  }
  __syncthreads();

  // ---- phase B: the candidates, one wave each -----------------------------------------------------------------------------
  const int ncand = S + (greedy_ids ? 1 : 0);
  for (int c = wave; c < ncand; c += kWaves) {
    const long* row = c < S ? ids + ((long)b * S + c) * T : greedy_ids + (long)b * Tg;
    int len = c < S ? (int)lengths[(long)b * S + c] : Tg;
    const int width = c < S ? T : Tg;
    len = len < 0 ? 0 : len > width ? width : len;
    const long t = lane < len ? row[lane] : end_id;
    const unsigned long long ends = __ballot(t == end_id);                 // lanes >= len count as <end>; len <= 64
    // the ids before the first <end>, within the length; the same in every lane, and said so (it bounds loops that read lanes)
    const int words = __builtin_amdgcn_readfirstlane(ends ? __ffsll(ends) - 1 : len);
    const int f0 = lane < words ? (int)field((int)t) : 0;
    const int f1 = __shfl_down(f0, 1, 64), f2 = __shfl_down(f0, 2, 64), f3 = __shfl_down(f0, 3, 64);
    uint64_t ck[kOrders];
    bool cv[kOrders];
    ck[0] = (uint64_t)f0;
    ck[1] = ck[0] | (uint64_t)f1 << 16;
    ck[2] = ck[1] | (uint64_t)f2 << 32;
    ck[3] = ck[2] | (uint64_t)f3 << 48;
#pragma unroll
    for (int n = 0; n < kOrders; ++n) {
      cv[n] = lane + n + 1 <= words;
      if (!cv[n]) ck[n] = 0;
    }
    int cdf[kOrders];
    table_df<kOrders>(tkeys, tdf, K, ck, cv, cdf);
    double cw[kOrders], cnorm[kOrders];
    bool cfirst[kOrders];
#pragma unroll
    for (int n = 0; n < kOrders; ++n) {
      int tf = 0, before = 0;
      for (int m = 0; m < words - n; ++m) {                                // m is wave-uniform
        const int same = lane_read(ck[n], m) == ck[n];
        tf += same;
        before += same & (m < lane);
      }
      cfirst[n] = cv[n] && before == 0;
      cw[n] = cv[n] ? tfidf(tf, cdf[n], log_docs) : 0.0;
      cnorm[n] = sqrt(wave_sum_f64(cfirst[n] ? cw[n] * cw[n] : 0.0));
    }
    const int clen = words > 1 ? words - 1 : 0;                             // length in bigrams
    // sum_r (penalty_r / (norm_c norm_r)) sum_lanes min(w_c, w_r) w_r, the lanes' sum taken last: every lane adds up its own n-gram's
    // scaled terms over the references in order, and each order costs one wave sum per candidate instead of one per reference
    double part[kOrders] = {0.0, 0.0, 0.0, 0.0};
    for (int r = 0; r < nref; ++r) {
      const int rwords = sh.words[r];
      const double delta = (double)(clen - (rwords > 1 ? rwords - 1 : 0));
      const double penalty = exp(-(delta * delta) * inv_two_sigma2);
#pragma unroll
      for (int n = 0; n < kOrders; ++n) {
        double rw = 0.0;                                                   // 0 if the reference lacks the n-gram
        for (int m = 0; m < rwords - n; ++m)
          if (sh.key[r][n][m] == ck[n] && cfirst[n]) rw = sh.w[r][n][m];
        double val = cfirst[n] ? fmin(cw[n], rw) * rw : 0.0;
        const double rnorm = sh.norm[r][n];
        if (cnorm[n] != 0.0 && rnorm != 0.0) val /= cnorm[n] * rnorm;
        part[n] += val * penalty;
      }
    }
    double acc[kOrders];
#pragma unroll
    for (int n = 0; n < kOrders; ++n) acc[n] = wave_sum_f64(part[n]);
    const double score = nref > 0 ? (((acc[0] + acc[1]) + acc[2]) + acc[3]) / 4.0 / (double)nref * 10.0 : 0.0;
    if (lane == 0) {
      score64[(long)b * (S + 1) + c] = score;
      if (c < S) reward[(long)b * S + c] = (float)score;
      else greedy_reward = (float)score;
    }
  }
  if (baseline == 0) return;
  __syncthreads();

  // ---- the baseline, as train.self_critical_advantage: from the float32 rewards, in double, rounded once ---------------------
  const float* mine = reward + (long)b * S;
  for (int s = tid; s < S; s += kThreads) {
    const double r = (double)mine[s];
    double base;
    if (baseline == 1) {
      base = (double)greedy_reward;
    } else {
      double sum = 0.0;
      for (int m = 0; m < S; ++m) sum += (double)mine[m];
      base = (sum - r) / (double)(S - 1);
    }
    advantage[(long)b * S + s] = (float)(r - base);
  }
}

}  // namespace

extern "C" int st_cider_reward(const long* keys, const int* df, long K, double log_num_docs, const int* refs, const int* ref_len,
                               const int* ref_count, int B, int R, int Tr, const long* ids, const long* lengths, int S, int T,
                               const long* greedy_ids, int Tg, long end_id, double sigma, int baseline, double* score64, float* reward,
                               float* advantage, void* stream) {
  ST_CHECK(B >= 1, "st_cider_reward: B must be >= 1 (got %d)", B);
  ST_CHECK(R >= 1 && R <= ST_CIDER_MAX_REFS, "st_cider_reward: R must be in [1, %d] references per image (got %d)", ST_CIDER_MAX_REFS, R);
  ST_CHECK(Tr >= 1 && Tr <= ST_CIDER_MAX_TOKENS, "st_cider_reward: reference rows hold 1 to %d tokens (got Tr = %d)", ST_CIDER_MAX_TOKENS, Tr);
  ST_CHECK(S >= 1, "st_cider_reward: S must be >= 1 (got %d)", S);
  ST_CHECK(T >= 1 && T <= ST_CIDER_MAX_TOKENS, "st_cider_reward: candidate rows hold 1 to %d tokens (got T = %d)", ST_CIDER_MAX_TOKENS, T);
  ST_CHECK(!greedy_ids || (Tg >= 1 && Tg <= ST_CIDER_MAX_TOKENS), "st_cider_reward: greedy rows hold 1 to %d tokens (got Tg = %d)",
           ST_CIDER_MAX_TOKENS, Tg);
  ST_CHECK(baseline >= 0 && baseline <= 2, "st_cider_reward: baseline must be 0 (none), 1 (greedy) or 2 (mean) (got %d)", baseline);
  ST_CHECK(baseline != 1 || greedy_ids, "st_cider_reward: baseline = greedy needs greedy_ids");
  ST_CHECK(baseline != 2 || S >= 2, "st_cider_reward: baseline = mean needs S >= 2 (got %d)", S);
  ST_CHECK(baseline == 0 || advantage, "st_cider_reward: a baseline needs the advantage buffer");
  ST_CHECK(K >= 0 && (K == 0 || (keys && df)), "st_cider_reward: the table needs keys and df (K = %ld)", K);
  ST_CHECK(log_num_docs >= 0.0, "st_cider_reward: log(num_docs) must be >= 0 (got %g)", log_num_docs);
  ST_CHECK(sigma > 0.0, "st_cider_reward: sigma must be > 0 (got %g)", sigma);
  ST_CHECK(end_id >= 0 && end_id <= 65534, "st_cider_reward: end_id must be in [0, 65534] (got %ld)", end_id);
  ST_CHECK(refs && ref_len && ref_count && ids && lengths && score64 && reward, "st_cider_reward: null argument");
  hipLaunchKernelGGL(cider_reward_kernel, dim3(B), dim3(kThreads), 0, (hipStream_t)stream, keys, df, K, log_num_docs, refs, ref_len,
                     ref_count, R, Tr, ids, lengths, S, T, greedy_ids, Tg, end_id, 1.0 / (2.0 * sigma * sigma), baseline, score64,
                     reward, advantage);
  ST_LAUNCH_CHECK();
  return 0;
}
