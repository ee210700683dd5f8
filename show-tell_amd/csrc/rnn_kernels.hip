// Recurrent-decoder kernels for gfx950: packed-sequence input gather, the per-timestep
// "skinny" MFMA GEMM with fused GRU / LSTM gate epilogues, the BPTT gate-gradient kernels,
// embedding scatter-add, cross-entropy, column sums.
//
// Replaces what the reference delegates to cuDNN's fused RNN and to torch ops:
//   rnn.py:29-31   embedding + cat + pack_padded_sequence      -> pack_inputs_kernel
//   rnn.py:32      nn.GRU over a PackedSequence (fwd + autograd) -> rnn_gemm_kernel<GRU_*>, gru_bwd_gates_kernel
//   rnn_lstm.py:30 nn.LSTM                                       -> rnn_gemm_kernel<LSTM_*>, lstm_bwd_gates_kernel
//   main.py:149    nn.CrossEntropyLoss (fwd + bwd)               -> ce_kernel
//
// The recurrent product h_{t-1} W_hh^T has only B_t <= batch rows, so it is launch/latency
// bound, not FLOP bound: one block owns 16 hidden units (all gates of those units) x 16 batch
// rows, operands go straight from L2 to MFMA fragments (no LDS: each fragment is used once),
// and the whole gate nonlinearity runs in the epilogue so a timestep is ONE launch.
#include "common.h"
#include "rnn_kernels.h"
#include "decoder_host.h"
#include "select.h"
#include <string.h>

namespace {

template <typename T> struct Mfma;
template <> struct Mfma<bf16_t> {
  static constexpr int EPC = 8;
  static __device__ __forceinline__ void run(const u32x4& a, const u32x4& b, f32x4& c) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(&a),
                                                *reinterpret_cast<const bf16x8*>(&b), c, 0, 0, 0);
  }
};
template <> struct Mfma<float> {
  static constexpr int EPC = 4;
  static __device__ __forceinline__ void run(const u32x4& a, const u32x4& b, f32x4& c) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[e]), __uint_as_float(b[e]), c, 0, 0, 0);
  }
};

// 4 consecutive elements of T <-> 4 floats
template <typename T> __device__ __forceinline__ void load4(const T* p, float* v);
template <> __device__ __forceinline__ void load4<float>(const float* p, float* v) {
  const f32x4 t = *reinterpret_cast<const f32x4*>(p);
  v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
}
template <> __device__ __forceinline__ void load4<bf16_t>(const bf16_t* p, float* v) {
  const u32x2 t = *reinterpret_cast<const u32x2*>(p);
  v[0] = __uint_as_float(t[0] << 16); v[1] = __uint_as_float(t[0] & 0xffff0000u);
  v[2] = __uint_as_float(t[1] << 16); v[3] = __uint_as_float(t[1] & 0xffff0000u);
}
template <typename T> __device__ __forceinline__ void store4(T* p, const float* v);
template <> __device__ __forceinline__ void store4<float>(float* p, const float* v) {
  *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
}
template <> __device__ __forceinline__ void store4<bf16_t>(bf16_t* p, const float* v) {
  *reinterpret_cast<u32x2*>(p) = u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
}

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---------------------------------------------------------------------------------------
// skinny GEMM  acc[g][m][n] = sum_k A[m][k] * W[g*gstride + n][k]   (+ optional second pair)
// ---------------------------------------------------------------------------------------
// BWD (fused BPTT cell): the NG "gates" are NG 16-unit tiles of ONE gate group (gstride = 16), so the unit bound is checked per
// tile, and the (A, W) pair has its own row count M2 <= M.  Its K = 3H / 4H rows are long and every byte comes through the
// CU's texture path, so the fragments are REQUESTED coalesced -- lane i asks for row i / 4, 16-byte piece i % 4 of the 16-row x
// 64-byte fragment: four lanes = 64 contiguous bytes, 16 requests per wave-instruction instead of 64 -- and put into MFMA
// order (lane q4 * 16 + r16 <- lane r16 * 4 + q4) in registers.
__device__ __forceinline__ u32x4 lane_gather(const u32x4& v, int src4) {
  return u32x4{(unsigned)__builtin_amdgcn_ds_bpermute(src4, (int)v[0]), (unsigned)__builtin_amdgcn_ds_bpermute(src4, (int)v[1]),
               (unsigned)__builtin_amdgcn_ds_bpermute(src4, (int)v[2]), (unsigned)__builtin_amdgcn_ds_bpermute(src4, (int)v[3])};
}
template <typename T, int NG, bool HAS_X, int MT, bool BWD = false>
__device__ __forceinline__ void skinny_mma(const RnnGemmArgs& a, int mbase, int n0, int r16, int q4, int kslice,
                                           f32x4 (&accH)[MT][NG], f32x4 (&accX)[MT][NG]) {
  constexpr int EPC = Mfma<T>::EPC;
  // K steps requested per round trip; the fused two-operand, two-row-tile form halves it to stay within 2 waves per SIMD
  // (260 -> ~170 VGPRs: two blocks per CU overlap instead of one)
  constexpr int UNR = BWD ? (MT + NG <= 4 ? 4 : 2) : (HAS_X && MT == 2) ? 2 : 4;
  const int lr = BWD ? q4 * 4 + (r16 >> 2) : r16, lq = BWD ? (r16 & 3) : q4;   // the row and the 16-byte piece this lane requests
  const int n = n0 + lr;
  const bool nok = n < a.N;
  // The kernel is latency bound (every fragment comes from L2), so bytes in flight per wave are the lever: K is split
  // over the block's 4 waves and a group of UNR K-steps of BOTH operand pairs (h W_hh and, in the fused form, x W_ih)
  // is requested before the first MFMA of the group -- one round trip per group.  With MT > 1 the block covers MT
  // 16-row tiles with the SAME weight fragments held in registers: the weights, the bulk of the L2 traffic when many
  // cells run in one launch, are fetched once per MT tiles.
  const bool hasH = a.A != nullptr, hasX = HAS_X && a.A2 != nullptr;
  const T* WH = reinterpret_cast<const T*>(a.W) + (long)n * a.ldw;
  const long gsH = (long)a.gstride * a.ldw;
  const T* WX = reinterpret_cast<const T*>(a.W2) + (long)n * a.ldw2;
  const long gsX = (long)a.gstride * a.ldw2;
  const T* AH[MT]; const T* AX[MT]; bool mok[MT], mokH[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = mbase + t * 16 + lr;
    mok[t] = m < a.M;
    mokH[t] = BWD ? m < a.M2 : mok[t];
    AH[t] = reinterpret_cast<const T*>(a.A) + (long)m * a.lda;
    long xrow = m;
    if (a.x_keys && (HAS_X || a.A)) {                  // greedy decode: the token of the previous step picks an embedding row
      int tok = 0;
      if (mok[t]) {
        tok = key_token(a.x_keys[m], a.x_V);
        if (a.ids_out && n0 == 0 && kslice == 0 && q4 == 0) a.ids_out[(long)m * a.ids_stride + a.ids_t] = tok;
      }
      if (HAS_X) xrow = tok;                           // fused cell: the x operand
      else AH[t] = reinterpret_cast<const T*>(a.A) + (long)tok * a.lda;   // split step: the A operand is the input half
    }
    AX[t] = reinterpret_cast<const T*>(a.A2) + xrow * a.lda2;
  }
  const int nsH = hasH ? (a.K + 4 * EPC - 1) / (4 * EPC) : 0, nsX = hasX ? (a.K2 + 4 * EPC - 1) / (4 * EPC) : 0;
  const int spwH = (nsH + 3) / 4, spwX = (nsX + 3) / 4;
  const int begH = kslice * spwH, endH = min(nsH, begH + spwH), begX = kslice * spwX, endX = min(nsX, begX + spwX);
  const int ngroups = max((endH - begH + UNR - 1) / UNR, (endX - begX + UNR - 1) / UNR);
  for (int gi = 0; gi < ngroups; ++gi) {
    u32x4 fa[MT][UNR], fw[UNR][NG], xa[MT][UNR], xw[UNR][NG];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int sH = begH + gi * UNR + u, kH = (sH * 4 + lq) * EPC;
      const bool okH = sH < endH && kH < a.K;
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        fa[t][u] = u32x4{0u, 0u, 0u, 0u};
        if (mokH[t] && okH) fa[t][u] = *reinterpret_cast<const u32x4*>(AH[t] + kH);
      }
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        fw[u][g] = u32x4{0u, 0u, 0u, 0u};
        if ((BWD ? n + g * 16 < a.N : nok) && okH) fw[u][g] = *reinterpret_cast<const u32x4*>(WH + g * gsH + kH);
      }
      if (HAS_X) {
        const int sX = begX + gi * UNR + u, kX = (sX * 4 + lq) * EPC;
        const bool okX = sX < endX && kX < a.K2;
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          xa[t][u] = u32x4{0u, 0u, 0u, 0u};
          if (mok[t] && okX) xa[t][u] = *reinterpret_cast<const u32x4*>(AX[t] + kX);
        }
#pragma unroll
        for (int g = 0; g < NG; ++g) {
          xw[u][g] = u32x4{0u, 0u, 0u, 0u};
          if ((BWD ? n + g * 16 < a.N : nok) && okX) xw[u][g] = *reinterpret_cast<const u32x4*>(WX + g * gsX + kX);
        }
      }
    }
    if (BWD) {
      const int src4 = (r16 * 4 + q4) * 4;
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
#pragma unroll
        for (int t = 0; t < MT; ++t) { fa[t][u] = lane_gather(fa[t][u], src4); xa[t][u] = lane_gather(xa[t][u], src4); }
#pragma unroll
        for (int g = 0; g < NG; ++g) { fw[u][g] = lane_gather(fw[u][g], src4); xw[u][g] = lane_gather(xw[u][g], src4); }
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u)
#pragma unroll
      for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          Mfma<T>::run(fw[u][g], fa[t][u], accH[t][g]);
          if (HAS_X) Mfma<T>::run(xw[u][g], xa[t][u], accX[t][g]);
        }
  }
}

// EPI 0: out_f32[m][n] (+)= acc (+bias)         (BPTT dh += dgh W_hh, generic small products)
// EPI 1: GRU gates (training fwd with precomputed gx, or decode with fused x-projection)
// EPI 2: LSTM gates
// DROP (inter-layer dropout, full GRU / LSTM cells only): h' goes to hout unchanged, for the recurrence, and hout2 -- the row the layer
// above reads as its input -- receives the dropped h': the stored value times the mask of csrc/dropout.h at (site, packed row, unit) of
// `drop`, the kernel's second argument.  In the plain forms that argument is an empty struct and the code is what it was.
template <typename T> __device__ __forceinline__ float storage_round(float v);          // v as a T in memory holds it
template <> __device__ __forceinline__ float storage_round<float>(float v) { return v; }
template <> __device__ __forceinline__ float storage_round<bf16_t>(float v) { return bf16_bits_to_f32(f32_to_bf16_bits(v)); }
template <typename T>
__device__ __forceinline__ void drop_units4(const RnnDropArgs& d, int cell, int m, int n, const float* h, float* out) {
  const DropWords w = drop_words(d.key, d.site[cell], d.row0[cell] + m, n >> 2);
#pragma unroll
  for (int e = 0; e < 4; ++e) out[e] = w.w[e] >= d.key.thr ? storage_round<T>(h[e]) * d.key.scale : 0.f;
}

struct RnnNoDrop {};                                     // the second kernel argument of the plain forms: nothing
template <bool DROP> struct DropParam { typedef RnnNoDrop type; };
template <> struct DropParam<true> { typedef RnnDropArgs type; };

template <typename T, int NG, int EPI, bool HAS_X, int MT, bool DROP = false>
__global__ __launch_bounds__(256) void rnn_gemm_kernel(RnnGemmBatch batch, typename DropParam<DROP>::type drop) {
  // block = MT x 16 rows x 16 units (all NG gates); its 4 waves each take a quarter of K and the partial
  // accumulators meet in LDS: one round of L2 latency per launch instead of four.  Wave t < MT then runs the
  // epilogue of row tile t.  blockIdx.z selects one of the launch's independent cells (kernel-argument segment).
  const RnnGemmArgs& a = batch.c[blockIdx.z];
  __shared__ f32x4 red[4][MT][2 * NG][64];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r16 = lane & 15, q4 = lane >> 4;
  const int n0 = blockIdx.x * 16, mbase = blockIdx.y * 16 * MT;
  if (mbase >= a.M || n0 >= a.N) return;            // the grid is sized for the launch's largest cell
  const int m0 = mbase + (wid < MT ? wid : 0) * 16;  // the row tile whose epilogue this wave owns
  f32x4 accH[MT][NG], accX[MT][NG];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int g = 0; g < NG; ++g) { accH[t][g] = f32x4{0.f, 0.f, 0.f, 0.f}; accX[t][g] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  // the epilogue operands (biases, precomputed x-projection, previous state) are requested BEFORE the fragment loads
  // so that they arrive under the same round trip
  const int pm = m0 + r16, pn = n0 + 4 * q4;
  const bool epi_ok = wid < MT && pm < a.M && pn < a.N;
  float ex[NG][4], eb[NG][4], es[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int e = 0; e < 4; ++e) { ex[g][e] = 0.f; eb[g][e] = 0.f; }
  if (epi_ok) {
    if (EPI == 0) {
      if (a.bias_h) load4<float>(a.bias_h + pn, eb[0]);
      if (a.accumulate) load4<float>(a.out_f32 + (long)pm * a.ldo + pn, es);
    } else {
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        load4<float>(a.bias_h + g * a.N + pn, eb[g]);
        if (HAS_X) load4<float>(a.bias_x + g * a.N + pn, ex[g]);
        else if (a.accumulate == kCellSplit) load4<float>(reinterpret_cast<const float*>(a.gx) + (long)pm * a.ldgx + g * a.N + pn, ex[g]);   // recurrent half, already holds b_hh
        else if (a.accumulate != kCellRawOut) load4<T>(reinterpret_cast<const T*>(a.gx) + (long)pm * a.ldgx + g * a.N + pn, ex[g]);   // already holds b_ih
      }
      const void* prev = EPI == 1 ? a.hprev : a.cprev;
      if (prev && a.accumulate != kCellRawOut) load4<T>(reinterpret_cast<const T*>(prev) + (long)pm * a.ldhp + pn, es);
    }
  }
  skinny_mma<T, NG, HAS_X, MT>(a, mbase, n0, r16, q4, wid, accH, accX);
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int g = 0; g < NG; ++g) { red[wid][t][g][lane] = accH[t][g]; if (HAS_X) red[wid][t][NG + g][lane] = accX[t][g]; }
  __syncthreads();
  if (wid >= MT) return;
  f32x4 sumH[NG], sumX[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    sumH[g] = red[0][wid][g][lane];
    if (HAS_X) sumX[g] = red[0][wid][NG + g][lane];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      sumH[g] += red[w][wid][g][lane];
      if (HAS_X) sumX[g] += red[w][wid][NG + g][lane];
    }
  }

  // lane owns row m = m0 + r16 and units n = n0 + 4*q4 + {0..3}
  const int m = m0 + r16, n = n0 + 4 * q4;
  if (m >= a.M || n >= a.N) return;
  const int H = a.N;
  if (EPI == 0) {
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = sumH[0][e] + eb[0][e] + es[e];
    if (a.hout) store4<T>(reinterpret_cast<T*>(a.hout) + (long)m * a.ldho + n, v);      // output in the storage type (ldho)
    else *reinterpret_cast<f32x4*>(a.out_f32 + (long)m * a.ldo + n) = f32x4{v[0], v[1], v[2], v[3]};
  } else if (!HAS_X && a.accumulate == kCellRawOut) {
    // recurrent half for the NEXT use of this layer's cell: gate sums + b_hh, fp32, [m][g * N + n]
#pragma unroll
    for (int g = 0; g < NG; ++g)
      *reinterpret_cast<f32x4*>(a.out_f32 + (long)m * a.ldo + g * a.N + n) =
          f32x4{sumH[g][0] + eb[g][0], sumH[g][1] + eb[g][1], sumH[g][2] + eb[g][2], sumH[g][3] + eb[g][3]};
  } else if (EPI == 1) {
    // r,z,n order (torch.nn.GRU): r = s(xr+hr), z = s(xz+hz), n = tanh(xn + r*(hn)), h' = (1-z) n + z h
    float xg[3][4];
    const float* hp = es;
    const bool split = !HAS_X && a.accumulate == kCellSplit;   // MFMA sums = input half (+ b_ih in eb), ex = recurrent half (+ b_hh)
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) xg[g][e] = split ? sumH[g][e] + eb[g][e] : (HAS_X ? sumX[g][e] : 0.f) + ex[g][e];
    float hn[4], r[4], z[4], nn[4], hnew[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float hr = split ? ex[0][e] : sumH[0][e] + eb[0][e], hz = split ? ex[1][e] : sumH[1][e] + eb[1][e];
      hn[e] = split ? ex[2][e] : sumH[2][e] + eb[2][e];
      hnew[e] = st_gru_unit(xg[0][e], xg[1][e], xg[2][e], hr, hz, hn[e], hp[e], r[e], z[e], nn[e]);
    }
    store4<T>(reinterpret_cast<T*>(a.hout) + (long)m * a.ldho + n, hnew);
    if constexpr (DROP) {
      if (a.hout2) { float hd[4]; drop_units4<T>(drop, blockIdx.z, m, n, hnew, hd); store4<T>(reinterpret_cast<T*>(a.hout2) + (long)m * a.ldho2 + n, hd); }
    } else {
      if (a.hout2) store4<T>(reinterpret_cast<T*>(a.hout2) + (long)m * a.ldho2 + n, hnew);
    }
    if (a.cache) {
      T* c = reinterpret_cast<T*>(a.cache) + (long)m * a.ldcache + n;
      store4<T>(c, r); store4<T>(c + H, z); store4<T>(c + 2 * H, nn); store4<T>(c + 3 * H, hn);
    }
  } else {
    // i,f,g,o order (torch.nn.LSTM): c' = f c + i g ; h' = o tanh(c')
    float pre[4][4];
    const float* cp = es;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) pre[g][e] = (HAS_X ? sumX[g][e] : 0.f) + ex[g < NG ? g : 0][e] + sumH[g < NG ? g : 0][e] + eb[g < NG ? g : 0][e];
    float ig[4], fg[4], gg[4], og[4], cn[4], hnew[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) hnew[e] = st_lstm_unit(pre[0][e], pre[1][e], pre[2][e], pre[3][e], cp[e], ig[e], fg[e], gg[e], og[e], cn[e]);
    store4<T>(reinterpret_cast<T*>(a.hout) + (long)m * a.ldho + n, hnew);
    if constexpr (DROP) {
      if (a.hout2) { float hd[4]; drop_units4<T>(drop, blockIdx.z, m, n, hnew, hd); store4<T>(reinterpret_cast<T*>(a.hout2) + (long)m * a.ldho2 + n, hd); }
    } else {
      if (a.hout2) store4<T>(reinterpret_cast<T*>(a.hout2) + (long)m * a.ldho2 + n, hnew);
    }
    store4<T>(reinterpret_cast<T*>(a.cout) + (long)m * a.ldho + n, cn);
    if (a.cache) {
      T* c = reinterpret_cast<T*>(a.cache) + (long)m * a.ldcache + n;
      store4<T>(c, ig); store4<T>(c + H, fg); store4<T>(c + 2 * H, gg); store4<T>(c + 3 * H, og);
    }
  }
}

// ---------------------------------------------------------------------------------------
// packed input rows: x0[row(t,b)] = t == 0 ? feat[b] : emb[caption[b][t-1]]   (rnn.py:29-31)
//                    target[row(t,b)] = caption[b][t]                          (main.py:145)
// mode 1 (attention decoder, rnn_attn.py:70): x0[row] = emb[caption[b][t]]
// `ids` ([B][Tcap]; the launcher passes cap when the caller has none) is what the rows embed, `cap` what the targets are
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void pack_inputs_kernel(const T* __restrict__ feat, const T* __restrict__ emb,
                                                          const long* __restrict__ cap, int Tcap,
                                                          const int* __restrict__ rows_b, const int* __restrict__ rows_t,
                                                          T* __restrict__ x0, long* __restrict__ target,
                                                          int ntok, int E, int V, int mode, const long* __restrict__ ids) {
  constexpr int N = 16 / (int)sizeof(T);
  const int cpr = E / N;
  const long total = (long)ntok * cpr;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int row = (int)(i / cpr), c = (int)(i - (long)row * cpr) * N;
    const int b = rows_b[row], t = rows_t[row];
    const T* src;
    if (mode == 0 && t == 0) src = feat + (long)b * E + c;
    else {
      long tok = ids[(long)b * Tcap + (mode == 0 ? t - 1 : t)];
      tok = tok < 0 ? 0 : (tok >= V ? V - 1 : tok);   // keep a corrupt id from faulting the GPU
      src = emb + tok * E + c;
    }
    *reinterpret_cast<u32x4*>(x0 + (long)row * E + c) = *reinterpret_cast<const u32x4*>(src);
    if (c == 0 && target) target[row] = cap[(long)b * Tcap + t];
  }
}

// dX0 rows -> dfeat (t == 0, plain store) and dEmb (t >= 1, fp32 atomics; 256 contiguous bytes per wave-instruction)
__global__ __launch_bounds__(256) void embedding_bwd_kernel(const float* __restrict__ dx0, const long* __restrict__ cap, int Tcap,
                                                            const int* __restrict__ rows_b, const int* __restrict__ rows_t,
                                                            float* __restrict__ dfeat, float* __restrict__ demb,
                                                            int ntok, int E, int V, int mode) {
  const long total = (long)ntok * E;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int row = (int)(i / E), c = (int)(i - (long)row * E);
    const int b = rows_b[row], t = rows_t[row];
    const float v = dx0[i];
    if (mode == 0 && t == 0) { if (dfeat) dfeat[(long)b * E + c] = v; }
    else {
      long tok = cap[(long)b * Tcap + (mode == 0 ? t - 1 : t)];
      tok = tok < 0 ? 0 : (tok >= V ? V - 1 : tok);
      atomicAdd(demb + tok * E + c, v);
    }
  }
}

// hprev[row(t,b)] = t == 0 ? h0 : y[row(t-1,b)]   (operand of dW_hh = sum_t dgh_t^T h_{t-1})
template <typename T>
__global__ __launch_bounds__(256) void gather_hprev_kernel(const T* __restrict__ y, const int* __restrict__ rows_t,
                                                           const int* __restrict__ prev_row, T* __restrict__ hp, int ntok, int H,
                                                           const T* __restrict__ h0, const int* __restrict__ rows_b) {
  constexpr int N = 16 / (int)sizeof(T);
  const int cpr = H / N;
  const long total = (long)ntok * cpr;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int row = (int)(i / cpr), c = (int)(i - (long)row * cpr) * N;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (rows_t[row] > 0) v = *reinterpret_cast<const u32x4*>(y + (long)prev_row[row] * H + c);
    else if (h0) v = *reinterpret_cast<const u32x4*>(h0 + (long)rows_b[row] * H + c);
    *reinterpret_cast<u32x4*>(hp + (long)row * H + c) = v;
  }
}

// GRU BPTT gate gradients for the B_t rows of one timestep (see DESIGN.md for the algebra)
template <typename T>
__global__ __launch_bounds__(256) void gru_bwd_gates_kernel(RnnBwdBatch batch, int H) {
  const RnnBwdCell& cl = batch.c[blockIdx.y];
  const float* __restrict__ dy = cl.dy; float* __restrict__ dhc = cl.dhc;
  const T* __restrict__ cache = reinterpret_cast<const T*>(cl.cache);
  const T* __restrict__ hprev = reinterpret_cast<const T*>(cl.hprev);
  T* __restrict__ dgx = reinterpret_cast<T*>(cl.dgx); T* __restrict__ dgh = reinterpret_cast<T*>(cl.dgh);
  const int Bt = cl.Bt;
  const int total = Bt * (H / 4);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int b = i / (H / 4), j = (i - b * (H / 4)) * 4;
  float g[4], c[4], r[4], z[4], n[4], hn[4], hp[4] = {0.f, 0.f, 0.f, 0.f};
  load4<float>(dy + (long)b * H + j, g);
  load4<float>(dhc + (long)b * H + j, c);
  const T* cr = cache + (long)b * 4 * H + j;
  load4<T>(cr, r); load4<T>(cr + H, z); load4<T>(cr + 2 * H, n); load4<T>(cr + 3 * H, hn);
  if (hprev) load4<T>(hprev + (long)b * H + j, hp);
  float drp[4], dzp[4], dnp[4], dnr[4], dhz[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float dh = g[e] + c[e];
    const float dn = dh * (1.f - z[e]);
    const float dz = dh * (hp[e] - n[e]);
    dnp[e] = dn * (1.f - n[e] * n[e]);
    drp[e] = dnp[e] * hn[e] * r[e] * (1.f - r[e]);
    dzp[e] = dz * z[e] * (1.f - z[e]);
    dnr[e] = dnp[e] * r[e];
    dhz[e] = dh * z[e];
  }
  T* ox = dgx + (long)b * 3 * H + j;
  T* oh = dgh + (long)b * 3 * H + j;
  store4<T>(ox, drp); store4<T>(ox + H, dzp); store4<T>(ox + 2 * H, dnp);
  store4<T>(oh, drp); store4<T>(oh + H, dzp); store4<T>(oh + 2 * H, dnr);
  store4<float>(dhc + (long)b * H + j, dhz);
}

// LSTM BPTT gate gradients: dg is shared by the x- and h-projections (all four gates are sums)
template <typename T>
__global__ __launch_bounds__(256) void lstm_bwd_gates_kernel(RnnBwdBatch batch, int H) {
  const RnnBwdCell& cl = batch.c[blockIdx.y];
  const float* __restrict__ dy = cl.dy; float* __restrict__ dhc = cl.dhc; float* __restrict__ dcc = cl.dcc;
  const T* __restrict__ cache = reinterpret_cast<const T*>(cl.cache);
  const T* __restrict__ cnew = reinterpret_cast<const T*>(cl.cnew);
  const T* __restrict__ cprev = reinterpret_cast<const T*>(cl.cprev);
  T* __restrict__ dg = reinterpret_cast<T*>(cl.dgx);
  const int Bt = cl.Bt;
  const int total = Bt * (H / 4);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int b = i / (H / 4), j = (i - b * (H / 4)) * 4;
  float g[4], ch[4], cc[4], ig[4], fg[4], gg[4], og[4], cn[4], cp[4] = {0.f, 0.f, 0.f, 0.f};
  load4<float>(dy + (long)b * H + j, g);
  load4<float>(dhc + (long)b * H + j, ch);
  load4<float>(dcc + (long)b * H + j, cc);
  const T* cr = cache + (long)b * 4 * H + j;
  load4<T>(cr, ig); load4<T>(cr + H, fg); load4<T>(cr + 2 * H, gg); load4<T>(cr + 3 * H, og);
  load4<T>(cnew + (long)b * H + j, cn);
  if (cprev) load4<T>(cprev + (long)b * H + j, cp);
  float di[4], df[4], dgg[4], dob[4], dcp[4], zero[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float dh = g[e] + ch[e];
    const float tc = tanhf(cn[e]);
    const float dc = cc[e] + dh * og[e] * (1.f - tc * tc);
    dob[e] = dh * tc * og[e] * (1.f - og[e]);
    di[e] = dc * gg[e] * ig[e] * (1.f - ig[e]);
    df[e] = dc * cp[e] * fg[e] * (1.f - fg[e]);
    dgg[e] = dc * ig[e] * (1.f - gg[e] * gg[e]);
    dcp[e] = dc * fg[e];
  }
  T* o = dg + (long)b * 4 * H + j;
  store4<T>(o, di); store4<T>(o + H, df); store4<T>(o + 2 * H, dgg); store4<T>(o + 3 * H, dob);
  store4<float>(dcc + (long)b * H + j, dcp);
  store4<float>(dhc + (long)b * H + j, zero);   // dh_{t-1} is entirely the GEMM term, accumulated next
}


// ---------------------------------------------------------------------------------------
// fused BPTT cell (pull form): dh = [dy] + dgh_{l,t+1} W_hh_l + dgx_{l+1,t} W_ih_{l+1} + dhc, then the gate gradients of
// gru_bwd_gates_kernel / lstm_bwd_gates_kernel (same expressions, same order) for the block's own rows and units.
// Block = MT x 16 rows x NT x 16 units; K is split over the 4 waves as in rnn_gemm_kernel, the partial sums meet in LDS
// and wave w runs the epilogue of the 16 x 16 tiles w, w + 4, ...  Every element of dhc / dcc is read and written by the
// same lane of the same block, and the products read only what the previous diagonal's launch wrote.
// ---------------------------------------------------------------------------------------
template <typename T> struct Raw4;                       // 4 consecutive elements as loaded: unpacked only in the epilogue
template <> struct Raw4<float> { typedef f32x4 type; };
template <> struct Raw4<bf16_t> { typedef u32x2 type; };
template <typename T> __device__ __forceinline__ void unpack4(const typename Raw4<T>::type& t, float* v);
template <> __device__ __forceinline__ void unpack4<float>(const f32x4& t, float* v) { v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3]; }
template <> __device__ __forceinline__ void unpack4<bf16_t>(const u32x2& t, float* v) {
  v[0] = __uint_as_float(t[0] << 16); v[1] = __uint_as_float(t[0] & 0xffff0000u);
  v[2] = __uint_as_float(t[1] << 16); v[3] = __uint_as_float(t[1] & 0xffff0000u);
}

// DROP (inter-layer dropout): the from-above product dgx_{l+1,t} W_ih_{l+1} is the gradient of the DROPPED y_l, so it takes the mask
// of csrc/dropout.h times scale before it joins the recurrent product, which is not masked.  Each lane's accX[t][g] is 4 consecutive units
// of one row: one Philox call per tile and lane, in registers, before the cross-wave reduction (the mask is the same in all 4 K slices).
template <typename T, bool LSTM, int MT, int NT, bool DROP = false>
__global__ __launch_bounds__(256) void rnn_bwd_cell_kernel(RnnBwdFusedBatch batch, typename DropParam<DROP>::type drop) {
  typedef typename Raw4<T>::type raw_t;
  const RnnGemmArgs& a = batch.c[blockIdx.z].g;
  const RnnBwdCell& c = batch.c[blockIdx.z].e;
  constexpr int TILES = MT * NT, TPW = (TILES + 3) / 4;
  __shared__ f32x4 red[4][TILES][64];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r16 = lane & 15, q4 = lane >> 4;
  const int n0 = blockIdx.x * 16 * NT, mbase = blockIdx.y * 16 * MT;
  if (mbase >= a.M || n0 >= a.N) return;            // the grid is sized for the launch's largest cell
  const int H = a.N;
  f32x4 accH[MT][NT], accX[MT][NT];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int g = 0; g < NT; ++g) { accH[t][g] = f32x4{0.f, 0.f, 0.f, 0.f}; accX[t][g] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  // the epilogue operands are requested BEFORE the fragment loads so that they arrive under the same round trip:
  // tile i = wid + 4 j is row tile i / NT, unit tile i % NT; the lane owns row pm and units pn .. pn + 3 of it
  bool ok[TPW]; int pm[TPW], pn[TPW];
  f32x4 rdy[TPW], rdhc[TPW], rdcc[TPW]; raw_t rc[TPW][4], rp[TPW], rcn[TPW];
  const T* cache = reinterpret_cast<const T*>(c.cache);
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    const int i = wid + 4 * j;
    pm[j] = mbase + (i / NT) * 16 + r16; pn[j] = n0 + (i % NT) * 16 + 4 * q4;
    ok[j] = i < TILES && pm[j] < a.M && pn[j] < H;
    rdy[j] = rdhc[j] = rdcc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    rp[j] = rcn[j] = raw_t{};
#pragma unroll
    for (int q = 0; q < 4; ++q) rc[j][q] = raw_t{};
    if (!ok[j]) continue;
    const long o = (long)pm[j] * H + pn[j];
    if (c.dy) rdy[j] = *reinterpret_cast<const f32x4*>(c.dy + o);
#pragma unroll
    for (int q = 0; q < 4; ++q) rc[j][q] = *reinterpret_cast<const raw_t*>(cache + (long)pm[j] * 4 * H + q * H + pn[j]);
    if (LSTM) {
      rdcc[j] = *reinterpret_cast<const f32x4*>(c.dcc + o);
      rcn[j] = *reinterpret_cast<const raw_t*>(reinterpret_cast<const T*>(c.cnew) + o);
      if (c.cprev) rp[j] = *reinterpret_cast<const raw_t*>(reinterpret_cast<const T*>(c.cprev) + o);
    } else {
      rdhc[j] = *reinterpret_cast<const f32x4*>(c.dhc + o);
      if (c.hprev) rp[j] = *reinterpret_cast<const raw_t*>(reinterpret_cast<const T*>(c.hprev) + o);
    }
  }
  skinny_mma<T, NT, true, MT, true>(a, mbase, n0, r16, q4, wid, accH, accX);
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int g = 0; g < NT; ++g) {
      if constexpr (DROP) {
        f32x4 mk = f32x4{1.f, 1.f, 1.f, 1.f};
        if (a.A2) {
          const DropWords w = drop_words(drop.key, drop.site[blockIdx.z], drop.row0[blockIdx.z] + mbase + t * 16 + r16, (n0 + g * 16) / 4 + q4);
          mk = f32x4{drop_mult(drop.key, w.w[0]), drop_mult(drop.key, w.w[1]), drop_mult(drop.key, w.w[2]), drop_mult(drop.key, w.w[3])};
        }
        red[wid][t * NT + g][lane] = accH[t][g] + mk * accX[t][g];
      } else {
        red[wid][t * NT + g][lane] = accH[t][g] + accX[t][g];
      }
    }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    if (!ok[j]) continue;
    const int i = wid + 4 * j;
    const f32x4 s = ((red[0][i][lane] + red[1][i][lane]) + red[2][i][lane]) + red[3][i][lane];
    const long o = (long)pm[j] * H + pn[j];
    if (!LSTM) {
      float r[4], z[4], n[4], hn[4], hp[4];
      unpack4<T>(rc[j][0], r); unpack4<T>(rc[j][1], z); unpack4<T>(rc[j][2], n); unpack4<T>(rc[j][3], hn); unpack4<T>(rp[j], hp);
      float drp[4], dzp[4], dnp[4], dnr[4], dhz[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float dh = (rdy[j][e] + rdhc[j][e]) + s[e];
        const float dn = dh * (1.f - z[e]);
        const float dz = dh * (hp[e] - n[e]);
        dnp[e] = dn * (1.f - n[e] * n[e]);
        drp[e] = dnp[e] * hn[e] * r[e] * (1.f - r[e]);
        dzp[e] = dz * z[e] * (1.f - z[e]);
        dnr[e] = dnp[e] * r[e];
        dhz[e] = dh * z[e];
      }
      T* ox = reinterpret_cast<T*>(c.dgx) + (long)pm[j] * 3 * H + pn[j];
      T* oh = reinterpret_cast<T*>(c.dgh) + (long)pm[j] * 3 * H + pn[j];
      store4<T>(ox, drp); store4<T>(ox + H, dzp); store4<T>(ox + 2 * H, dnp);
      store4<T>(oh, drp); store4<T>(oh + H, dzp); store4<T>(oh + 2 * H, dnr);
      store4<float>(c.dhc + o, dhz);
    } else {
      float ig[4], fg[4], gg[4], og[4], cn[4], cp[4];
      unpack4<T>(rc[j][0], ig); unpack4<T>(rc[j][1], fg); unpack4<T>(rc[j][2], gg); unpack4<T>(rc[j][3], og);
      unpack4<T>(rcn[j], cn); unpack4<T>(rp[j], cp);
      float di[4], df[4], dgg[4], dob[4], dcp[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float dh = rdy[j][e] + s[e];            // dh_t of the LSTM is entirely the two products (+ dy at the top)
        const float tc = tanhf(cn[e]);
        const float dc = rdcc[j][e] + dh * og[e] * (1.f - tc * tc);
        dob[e] = dh * tc * og[e] * (1.f - og[e]);
        di[e] = dc * gg[e] * ig[e] * (1.f - ig[e]);
        df[e] = dc * cp[e] * fg[e] * (1.f - fg[e]);
        dgg[e] = dc * ig[e] * (1.f - gg[e] * gg[e]);
        dcp[e] = dc * fg[e];
      }
      T* og_ = reinterpret_cast<T*>(c.dgx) + (long)pm[j] * 4 * H + pn[j];
      store4<T>(og_, di); store4<T>(og_ + H, df); store4<T>(og_ + 2 * H, dgg); store4<T>(og_ + 3 * H, dob);
      store4<float>(c.dcc + o, dcp);
    }
  }
}

// ---------------------------------------------------------------------------------------
// cross entropy over rows (mean reduction):  loss += -log softmax(x)[t] / nrows
// dlogits = (softmax - onehot) * gscale   written in TD (may alias the logits when TD == TL)
// one block per row; the row is read twice from L2 (max+sum online, then gradient)
// WGT: the row's loss term and gradient are also times row_w[row] (NULL: 1; the divisor stays nrows) and its unweighted
// -log softmax(x)[t] goes to nll[row] (NULL: not stored); without WGT the kernel is the code it was
// LS (label smoothing, with WGT): the first pass also carries sum x beside (m, s); u = lse - sum / V goes to smooth[row] (NULL: not
// stored), the row's term is (1 - eps) * nll + eps * u and dlogits = (softmax - (1 - eps) * onehot - eps / V) * gscale; every read of
// the row that the loss needs still happens before the first write.  The other instantiations are the code they were
// ---------------------------------------------------------------------------------------
struct CeSmooth {
  float* smooth;   // [rows] or NULL
  float eps, inv_v;
};
template <typename TL, typename TD, bool WGT, bool LS = false>
__global__ __launch_bounds__(256) void ce_kernel(const TL* __restrict__ logits, const long* __restrict__ target,
                                                 float* __restrict__ loss, TD* __restrict__ dlogits,
                                                 int V, int ldl, int ldd, float inv_rows, float gscale, const float* __restrict__ gscale_dev,
                                                 const float* __restrict__ row_w, float* __restrict__ nll, CeSmooth ls) {
  __shared__ float sm[8], ss[8];
  __shared__ float sx[LS ? 8 : 1];
  const int row = blockIdx.x;
  const TL* x = logits + (long)row * ldl;
  float m = -INFINITY, s = 0.f, xs = 0.f;
  for (int i = threadIdx.x; i < V; i += blockDim.x) {
    const float v = to_f32<TL>(x[i]);
    const float nm = fmaxf(m, v);
    if constexpr (LS) {   // the fused multiply-add spelled out: beside `xs += v` the compiler pairs the two additions instead of contracting
      s = __fmaf_rn(s, __expf(m - nm), __expf(v - nm));   // this one, and lse would differ from the other instantiations' in its last bit
      xs += v;
    } else {
      s = s * __expf(m - nm) + __expf(v - nm);
    }
    m = nm;
  }
  // combine (m, s) pairs across the wave, then across waves
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64), os = __shfl_xor(s, o, 64);
    const float nm = fmaxf(m, om);
    s = (m == -INFINITY ? 0.f : s * __expf(m - nm)) + (om == -INFINITY ? 0.f : os * __expf(om - nm));
    m = nm;
    if constexpr (LS) xs += __shfl_xor(xs, o, 64);
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) { sm[wid] = m; ss[wid] = s; }
  if constexpr (LS) { if (lane == 0) sx[wid] = xs; }
  __syncthreads();
  float M = sm[0], S = ss[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) {
    const float nm = fmaxf(M, sm[w]);
    S = S * __expf(M - nm) + ss[w] * __expf(sm[w] - nm);
    M = nm;
  }
  float X = 0.f;
  if constexpr (LS) { for (int w = 0; w < (int)(blockDim.x >> 6); ++w) X += sx[w]; }
  long t = target[row];
  t = t < 0 ? 0 : (t >= V ? V - 1 : t);
  const float lse = M + __logf(S);
  const float xt = to_f32<TL>(x[t]);
  __syncthreads();   // dlogits may alias the logits: every read of x[t] happens before any write
  float keep = 1.f, unif = 0.f;
  if constexpr (LS) {
    const float wr = row_w ? row_w[row] : 1.f;
    const float nl = lse - xt, u = lse - X * ls.inv_v;
    keep = 1.f - ls.eps; unif = ls.eps * ls.inv_v;
    if (threadIdx.x == 0 && nll) nll[row] = nl;
    if (threadIdx.x == 0 && ls.smooth) ls.smooth[row] = u;
    if (threadIdx.x == 0 && loss) atomicAdd(loss, wr * (keep * nl + ls.eps * u) * inv_rows);
    gscale *= wr;
  } else if constexpr (WGT) {
    const float wr = row_w ? row_w[row] : 1.f;
    if (threadIdx.x == 0 && nll) nll[row] = lse - xt;
    if (threadIdx.x == 0 && loss) atomicAdd(loss, wr * (lse - xt) * inv_rows);
    gscale *= wr;
  } else {
    if (threadIdx.x == 0 && loss) atomicAdd(loss, (lse - xt) * inv_rows);
  }
  if (dlogits) {
    if (gscale_dev) gscale *= *gscale_dev;
    TD* d = dlogits + (long)row * ldd;
    for (int i = threadIdx.x; i < V; i += blockDim.x) {
      const float p = __expf(to_f32<TL>(x[i]) - lse);
      if constexpr (LS) d[i] = from_f32<TD>((p - ((i == t ? keep : 0.f) + unif)) * gscale);
      else d[i] = from_f32<TD>((p - (i == t ? 1.f : 0.f)) * gscale);
    }
    for (int i = V + threadIdx.x; i < ldd; i += blockDim.x) d[i] = from_f32<TD>(0.f);   // pad columns feed GEMMs as K
  }
}

// out[n] += sum_rows x[row][n]      (bias gradients); one thread per column, coalesced over n
template <typename T>
__global__ __launch_bounds__(256) void colsum_kernel(const T* __restrict__ x, float* __restrict__ out, int rows, int cols, int ldx, int rows_per_block) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= cols) return;
  const int r0 = blockIdx.y * rows_per_block, r1 = min(rows, r0 + rows_per_block);
  float s = 0.f;
  for (int r = r0; r < r1; ++r) s += to_f32<T>(x[(long)r * ldx + n]);
  atomicAdd(out + n, s);
}

}  // namespace

// ---------------------------------------------------------------------------------------
// internal launchers (declared in rnn_kernels.h)
// ---------------------------------------------------------------------------------------
// drop (NULL: the plain forms): the DROP forms of a forward diagonal -- full cells (has_x) with a gate epilogue, at most one per layer,
// none empty, because drop->site / drop->row0 are indexed like `cells`
static int gemm_launch(const RnnGemmArgs* cells, int ncells, int dtype, int epi, int has_x, const RnnDropArgs* drop, hipStream_t st) {
  ST_CHECK(ncells >= 0 && ncells <= kRnnBatch, "rnn_gemm: %d cells in one launch (max %d)", ncells, kRnnBatch);
  ST_CHECK(!drop || (ncells <= ST_MAX_LAYERS && has_x && (epi == 1 || epi == 2)), "rnn_gemm(drop): full gate cells only, at most %d", ST_MAX_LAYERS);
  RnnGemmBatch b;
  memset(&b, 0, sizeof(b));
  const int epc = dtype == ST_BF16 ? 8 : 4;
  int nc = 0, maxM = 0, maxN = 0;
  for (int i = 0; i < ncells; ++i) {
    const RnnGemmArgs& a = cells[i];
    if (a.M <= 0) { ST_CHECK(!drop, "rnn_gemm(drop): empty cell"); continue; }
    ST_CHECK(a.N % 4 == 0, "rnn_gemm: N=%d must be a multiple of 4", a.N);
    ST_CHECK(a.K % epc == 0 && a.lda % epc == 0 && a.ldw % epc == 0, "rnn_gemm: K/lda/ldw must be multiples of %d", epc);
    if (has_x) ST_CHECK(a.K2 % epc == 0 && a.lda2 % epc == 0 && a.ldw2 % epc == 0, "rnn_gemm: K2/lda2/ldw2 must be multiples of %d", epc);
    b.c[nc++] = a;
    if (a.M > maxM) maxM = a.M;
    if (a.N > maxN) maxN = a.N;
  }
  if (nc == 0) return 0;
  const dim3 grid((maxN + 15) / 16, (maxM + 15) / 16, nc), block(256);
  // many cells in one launch: the weights are most of the L2 traffic -> two row tiles per block share them
  // ... and so do the 16-row tiles of one tall cell (beam search steps 1280 rows at a time: 80 row tiles re-read the weights)
  const bool mt2 = (nc >= 2 || maxM >= 512) && maxM > 16;
  const dim3 grid2((maxN + 15) / 16, (maxM + 31) / 32, nc);
#define RG(T, NG, EPI, HX) do { if (mt2) hipLaunchKernelGGL((rnn_gemm_kernel<T, NG, EPI, HX, 2>), grid2, block, 0, st, b, RnnNoDrop{}); \
                               else hipLaunchKernelGGL((rnn_gemm_kernel<T, NG, EPI, HX, 1>), grid, block, 0, st, b, RnnNoDrop{}); } while (0)
#define RGD(T, NG, EPI) do { if (mt2) hipLaunchKernelGGL((rnn_gemm_kernel<T, NG, EPI, true, 2, true>), grid2, block, 0, st, b, *drop); \
                            else hipLaunchKernelGGL((rnn_gemm_kernel<T, NG, EPI, true, 1, true>), grid, block, 0, st, b, *drop); } while (0)
  if (drop) {
    if (dtype == ST_BF16) { if (epi == 1) RGD(bf16_t, 3, 1); else RGD(bf16_t, 4, 2); }
    else { if (epi == 1) RGD(float, 3, 1); else RGD(float, 4, 2); }
  } else if (dtype == ST_BF16) {
    if (epi == 0) RG(bf16_t, 1, 0, false);
    else if (epi == 1) { if (has_x) RG(bf16_t, 3, 1, true); else RG(bf16_t, 3, 1, false); }
    else { if (has_x) RG(bf16_t, 4, 2, true); else RG(bf16_t, 4, 2, false); }
  } else {
    if (epi == 0) RG(float, 1, 0, false);
    else if (epi == 1) { if (has_x) RG(float, 3, 1, true); else RG(float, 3, 1, false); }
    else { if (has_x) RG(float, 4, 2, true); else RG(float, 4, 2, false); }
  }
#undef RG
#undef RGD
  ST_LAUNCH_CHECK();
  return 0;
}

int rnn_gemm_launch_batch(const RnnGemmArgs* cells, int ncells, int dtype, int epi, int has_x, hipStream_t st) {
  return gemm_launch(cells, ncells, dtype, epi, has_x, nullptr, st);
}
int rnn_gemm_launch_batch_drop(const RnnGemmArgs* cells, int ncells, int dtype, int epi, const RnnDropArgs& drop, hipStream_t st) {
  return gemm_launch(cells, ncells, dtype, epi, 1, &drop, st);
}

int rnn_gemm_launch(const RnnGemmArgs& a, int dtype, int epi, int has_x, hipStream_t st) {
  return rnn_gemm_launch_batch(&a, 1, dtype, epi, has_x, st);
}

int rnn_bwd_gates_launch_batch(const RnnBwdCell* cells, int ncells, int H, int cell_kind, int dtype, hipStream_t st) {
  ST_CHECK(ncells >= 0 && ncells <= kRnnBatch, "rnn_bwd_gates: %d cells in one launch (max %d)", ncells, kRnnBatch);
  RnnBwdBatch b;
  memset(&b, 0, sizeof(b));
  int nc = 0, maxB = 0;
  for (int i = 0; i < ncells; ++i) {
    if (cells[i].Bt <= 0) continue;
    b.c[nc++] = cells[i];
    if (cells[i].Bt > maxB) maxB = cells[i].Bt;
  }
  if (nc == 0) return 0;
  const dim3 grid((maxB * (H / 4) + 255) / 256, nc);
  if (cell_kind == ST_CELL_GRU) {
    if (dtype == ST_BF16) hipLaunchKernelGGL(gru_bwd_gates_kernel<bf16_t>, grid, dim3(256), 0, st, b, H);
    else hipLaunchKernelGGL(gru_bwd_gates_kernel<float>, grid, dim3(256), 0, st, b, H);
  } else {
    if (dtype == ST_BF16) hipLaunchKernelGGL(lstm_bwd_gates_kernel<bf16_t>, grid, dim3(256), 0, st, b, H);
    else hipLaunchKernelGGL(lstm_bwd_gates_kernel<float>, grid, dim3(256), 0, st, b, H);
  }
  ST_LAUNCH_CHECK();
  return 0;
}

// One launch for the cells of a reversed diagonal.  Block shape: 32 rows x 32 units, the fastest of 32 x 16, 32 x 32, 32 x 64,
// 64 x 32 and 64 x 64 at the bench shape (profiles/r05_bptt_tile_shapes.txt): larger blocks halve the operand bytes but leave
// CUs without a block and lengthen the K chain of every wave.
static int bwd_fused_launch(const RnnBwdFused* cells, int ncells, int cell_kind, int dtype, const RnnDropArgs* drop, hipStream_t st) {
  ST_CHECK(ncells >= 0 && ncells <= ST_MAX_LAYERS, "rnn_bwd_fused: %d cells in one launch (max %d)", ncells, ST_MAX_LAYERS);
  RnnBwdFusedBatch b;
  memset(&b, 0, sizeof(b));
  const int epc = dtype == ST_BF16 ? 8 : 4;
  int nc = 0, maxM = 0, maxN = 0;
  for (int i = 0; i < ncells; ++i) {
    const RnnGemmArgs& a = cells[i].g;
    if (a.M <= 0) { ST_CHECK(!drop, "rnn_bwd_fused(drop): empty cell"); continue; }   // drop is indexed like `cells`: no compaction
    ST_CHECK(a.N % 8 == 0, "rnn_bwd_fused: H=%d must be a multiple of 8", a.N);
    ST_CHECK(!a.A || (a.K % epc == 0 && a.lda % epc == 0 && a.ldw % epc == 0 && a.M2 >= 0 && a.M2 <= a.M),
             "rnn_bwd_fused: bad recurrent operand pair");
    ST_CHECK(!a.A2 || (a.K2 % epc == 0 && a.lda2 % epc == 0 && a.ldw2 % epc == 0), "rnn_bwd_fused: bad input operand pair");
    b.c[nc] = cells[i];
    b.c[nc].g.gstride = 16;                         // the "gates" of skinny_mma are the block's 16-unit tiles
    if (!a.A) b.c[nc].g.M2 = 0;
    ++nc;
    if (a.M > maxM) maxM = a.M;
    if (a.N > maxN) maxN = a.N;
  }
  if (nc == 0) return 0;
  const bool lstm = cell_kind == ST_CELL_LSTM;
  constexpr int MT = 2, NT = 2;
  const dim3 grid((maxN + 16 * NT - 1) / (16 * NT), (maxM + 16 * MT - 1) / (16 * MT), nc), block(256);
  if (drop) {
    if (dtype == ST_BF16) {
      if (lstm) hipLaunchKernelGGL((rnn_bwd_cell_kernel<bf16_t, true, MT, NT, true>), grid, block, 0, st, b, *drop);
      else hipLaunchKernelGGL((rnn_bwd_cell_kernel<bf16_t, false, MT, NT, true>), grid, block, 0, st, b, *drop);
    } else {
      if (lstm) hipLaunchKernelGGL((rnn_bwd_cell_kernel<float, true, MT, NT, true>), grid, block, 0, st, b, *drop);
      else hipLaunchKernelGGL((rnn_bwd_cell_kernel<float, false, MT, NT, true>), grid, block, 0, st, b, *drop);
    }
  } else if (dtype == ST_BF16) {
    if (lstm) hipLaunchKernelGGL((rnn_bwd_cell_kernel<bf16_t, true, MT, NT>), grid, block, 0, st, b, RnnNoDrop{});
    else hipLaunchKernelGGL((rnn_bwd_cell_kernel<bf16_t, false, MT, NT>), grid, block, 0, st, b, RnnNoDrop{});
  } else {
    if (lstm) hipLaunchKernelGGL((rnn_bwd_cell_kernel<float, true, MT, NT>), grid, block, 0, st, b, RnnNoDrop{});
    else hipLaunchKernelGGL((rnn_bwd_cell_kernel<float, false, MT, NT>), grid, block, 0, st, b, RnnNoDrop{});
  }
  ST_LAUNCH_CHECK();
  return 0;
}

int rnn_bwd_fused_launch_batch(const RnnBwdFused* cells, int ncells, int cell_kind, int dtype, hipStream_t st) {
  return bwd_fused_launch(cells, ncells, cell_kind, dtype, nullptr, st);
}
int rnn_bwd_fused_launch_batch_drop(const RnnBwdFused* cells, int ncells, int cell_kind, int dtype, const RnnDropArgs& drop, hipStream_t st) {
  return bwd_fused_launch(cells, ncells, cell_kind, dtype, &drop, st);
}

static inline int grid1d(long work, int threads = 256) {
  long b = (work + threads - 1) / threads;
  return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

int pack_inputs_launch(const void* feat, const void* emb, const long* cap, int Tcap, const int* rows_b, const int* rows_t,
                       void* x0, long* target, int ntok, int E, int V, int mode, int dtype, hipStream_t st, const long* ids) {
  if (ntok <= 0) return 0;
  if (!ids) ids = cap;
  const int n = dtype == ST_BF16 ? 8 : 4;
  ST_CHECK(E % n == 0, "pack_inputs: E=%d must be a multiple of %d", E, n);
  const int grid = grid1d((long)ntok * (E / n));
  if (dtype == ST_BF16) hipLaunchKernelGGL(pack_inputs_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, (const bf16_t*)feat, (const bf16_t*)emb, cap, Tcap, rows_b, rows_t, (bf16_t*)x0, target, ntok, E, V, mode, ids);
  else hipLaunchKernelGGL(pack_inputs_kernel<float>, dim3(grid), dim3(256), 0, st, (const float*)feat, (const float*)emb, cap, Tcap, rows_b, rows_t, (float*)x0, target, ntok, E, V, mode, ids);
  ST_LAUNCH_CHECK();
  return 0;
}

int embedding_bwd_launch(const float* dx0, const long* cap, int Tcap, const int* rows_b, const int* rows_t,
                         float* dfeat, float* demb, int ntok, int E, int V, int mode, hipStream_t st) {
  if (ntok <= 0) return 0;
  hipLaunchKernelGGL(embedding_bwd_kernel, dim3(grid1d((long)ntok * E)), dim3(256), 0, st, dx0, cap, Tcap, rows_b, rows_t, dfeat, demb, ntok, E, V, mode);
  ST_LAUNCH_CHECK();
  return 0;
}

int gather_hprev_launch(const void* y, const int* rows_t, const int* prev_row, void* hp, int ntok, int H, int dtype, hipStream_t st,
                        const void* h0, const int* rows_b) {
  if (ntok <= 0) return 0;
  const int n = dtype == ST_BF16 ? 8 : 4;
  ST_CHECK(H % n == 0, "gather_hprev: H=%d must be a multiple of %d", H, n);
  const int grid = grid1d((long)ntok * (H / n));
  if (dtype == ST_BF16) hipLaunchKernelGGL(gather_hprev_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, (const bf16_t*)y, rows_t, prev_row, (bf16_t*)hp, ntok, H, (const bf16_t*)h0, rows_b);
  else hipLaunchKernelGGL(gather_hprev_kernel<float>, dim3(grid), dim3(256), 0, st, (const float*)y, rows_t, prev_row, (float*)hp, ntok, H, (const float*)h0, rows_b);
  ST_LAUNCH_CHECK();
  return 0;
}

int gru_bwd_gates_launch(const float* dy, float* dhc, const void* cache, const void* hprev, void* dgx, void* dgh,
                         int Bt, int H, int dtype, hipStream_t st) {
  RnnBwdCell c;
  memset(&c, 0, sizeof(c));
  c.dy = dy; c.dhc = dhc; c.cache = cache; c.hprev = hprev; c.dgx = dgx; c.dgh = dgh; c.Bt = Bt;
  return rnn_bwd_gates_launch_batch(&c, 1, H, ST_CELL_GRU, dtype, st);
}

int lstm_bwd_gates_launch(const float* dy, float* dhc, float* dcc, const void* cache, const void* cnew, const void* cprev,
                          void* dg, int Bt, int H, int dtype, hipStream_t st) {
  RnnBwdCell c;
  memset(&c, 0, sizeof(c));
  c.dy = dy; c.dhc = dhc; c.dcc = dcc; c.cache = cache; c.cnew = cnew; c.cprev = cprev; c.dgx = dg; c.Bt = Bt;
  return rnn_bwd_gates_launch_batch(&c, 1, H, ST_CELL_LSTM, dtype, st);
}

int colsum_launch(const void* x, float* out, int rows, int cols, int ldx, int dtype, hipStream_t st) {
  if (rows <= 0 || cols <= 0) return 0;
  const int rpb = 64;
  const dim3 grid((cols + 255) / 256, (rows + rpb - 1) / rpb);
  if (dtype == ST_BF16) hipLaunchKernelGGL(colsum_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)x, out, rows, cols, ldx, rpb);
  else hipLaunchKernelGGL(colsum_kernel<float>, grid, dim3(256), 0, st, (const float*)x, out, rows, cols, ldx, rpb);
  ST_LAUNCH_CHECK();
  return 0;
}

namespace {
template <bool WGT, bool LS = false>
void ce_launch(const void* logits, int logits_dtype, const long* target, int rows, int V, int ldl, float* loss_accum, void* dlogits,
               int dlogits_dtype, int ldd, float inv, float gs, const float* grad_scale_dev, const float* row_w, float* nll, hipStream_t st,
               CeSmooth ls = CeSmooth{}) {
  const dim3 grid(rows), block(256);
  if (logits_dtype == ST_F32 && (dlogits_dtype == ST_F32 || !dlogits))
    hipLaunchKernelGGL((ce_kernel<float, float, WGT, LS>), grid, block, 0, st, (const float*)logits, target, loss_accum, (float*)dlogits, V, ldl, ldd, inv, gs, grad_scale_dev, row_w, nll, ls);
  else if (logits_dtype == ST_F32)
    hipLaunchKernelGGL((ce_kernel<float, bf16_t, WGT, LS>), grid, block, 0, st, (const float*)logits, target, loss_accum, (bf16_t*)dlogits, V, ldl, ldd, inv, gs, grad_scale_dev, row_w, nll, ls);
  else if (dlogits_dtype == ST_BF16 || !dlogits)
    hipLaunchKernelGGL((ce_kernel<bf16_t, bf16_t, WGT, LS>), grid, block, 0, st, (const bf16_t*)logits, target, loss_accum, (bf16_t*)dlogits, V, ldl, ldd, inv, gs, grad_scale_dev, row_w, nll, ls);
  else
    hipLaunchKernelGGL((ce_kernel<bf16_t, float, WGT, LS>), grid, block, 0, st, (const bf16_t*)logits, target, loss_accum, (float*)dlogits, V, ldl, ldd, inv, gs, grad_scale_dev, row_w, nll, ls);
}
}  // namespace

// nn.CrossEntropyLoss() on logits rows, forward and / or backward, with the terms of st_loss_terms (NULL: the plain mean).  Instantiations:
// smoothing = 0 with row_weight or nll_out -> WGT; smoothing = 0 with neither -> the plain kernel; smoothing = 1 -> WGT + LS at any eps
extern "C" int st_cross_entropy(const void* logits, int logits_dtype, const long* target, int rows, int V, int ldl,
                                const st_loss_terms* terms, float* loss_accum, void* dlogits, int dlogits_dtype, int ldd,
                                float grad_scale, const float* grad_scale_dev, void* stream) {
  const st_loss_terms t = terms ? *terms : st_loss_terms{};
  ST_CHECK(logits && target, "st_cross_entropy: null pointer");
  ST_CHECK(rows >= 0 && V > 0 && ldl >= V, "st_cross_entropy: bad shape");
  if (st_check_loss_terms(&t, "st_cross_entropy")) return 1;
  if (rows == 0) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const float inv = 1.0f / rows, gs = grad_scale / rows;
  if (!t.smoothing && (t.row_weight || t.nll_out))
    ce_launch<true>(logits, logits_dtype, target, rows, V, ldl, loss_accum, dlogits, dlogits_dtype, ldd, inv, gs, grad_scale_dev, t.row_weight, t.nll_out, st);
  else if (!t.smoothing)
    ce_launch<false>(logits, logits_dtype, target, rows, V, ldl, loss_accum, dlogits, dlogits_dtype, ldd, inv, gs, grad_scale_dev, nullptr, nullptr, st);
  else
    ce_launch<true, true>(logits, logits_dtype, target, rows, V, ldl, loss_accum, dlogits, dlogits_dtype, ldd, inv, gs, grad_scale_dev, t.row_weight,
                          t.nll_out, st, CeSmooth{t.smooth_out, t.label_smoothing, 1.0f / V});
  ST_LAUNCH_CHECK();
  return 0;
}
