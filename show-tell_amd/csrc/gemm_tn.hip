// Token-contraction GEMM, bf16 -> fp32, grouped:  C_g[M_g][N_g] (+)= A_g^T B_g  with A_g [K_g][lda] and B_g [K_g][ldb] row-major,
// i.e. the contraction index (the token of a packed sequence) is the SLOW axis of both operands as the decoder stores them.
// These are the parameter gradients of the decoder backward (autograd of nn.Linear / nn.GRU / nn.LSTM, main.py:151):
// dW_lin += dlogits^T y_top and dW_ih_l += dgx_l^T x_l, dW_hh_l += dgh_l^T h_{t-1}.  st_gemm_nt wants both operands K-major and so
// needed a transposed copy of each; here both tiles are loaded as they lie (16-byte row pieces, coalesced) into one LDS image
// (csrc/tn_tile.h) and reach the MFMAs through ds_read_b64_tr_b16, which hands a row-major block to the lanes column-major.
//
//   * one workgroup (256 threads, 4 waves as 2 x 2, 64 x 64 outputs each) owns a 128 x 128 output tile over the whole of K:
//     a fixed summation order per output, no atomics, so two identical calls give bit-identical results;
//   * K advances 64 rows (two images per operand) per barrier; the next step's rows are in flight in registers while the MFMAs
//     of this one run, and the LDS images are double-buffered (one barrier per step);
//   * rows k >= K, columns >= M / N and gathered rows that are absent are ZERO in LDS: the transposed read needs every lane of
//     the wave (EXEC all ones), so tails are padded, never branched around.  Pad columns of A / B may hold anything (NaN
//     included): column m of A reaches only row m of the product, which is not stored for m >= M;
//   * B's rows may be gathered: row k is B[b_row[k]], zero where b_row[k] < 0 or b_live[k] <= 0 -- h_{t-1} of every token straight
//     out of the layer output (st_packed_seq.prev_row / rows_t), as st_transpose_batch gathered it;
//   * the workgroups of the first N tile also add up the columns of A over their K walk (the bias gradients): per thread in
//     row order, then 16 partial sums per column in thread order -- no atomics, no extra launch.
#include "common.h"
#include "tn_tile.h"
#include <string.h>
#include <type_traits>

namespace {

constexpr int kMaxGroups = 12;
constexpr int kImages = 2;                        // images (of TN_BK rows) per operand and step
constexpr int kStep = kImages * TN_BK;            // rows of K per barrier
constexpr int kRowsPerThread = kStep / 16;        // 256 threads: thread t loads chunk t & 15 of rows (t >> 4) + 16 i

struct TnGroup {
  const bf16_t* a; const bf16_t* b; float* c;
  const int* b_row; const int* b_live;
  float* cs0; float* cs1;
  int M, N, K, lda, ldb, ldc, accumulate;
  int tile0, ntn;                                 // first tile of the group in the launch, N tiles per row block
};
struct TnArgs { TnGroup g[kMaxGroups]; int ng, ntiles; };

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

__device__ __forceinline__ bf16x8 tr_frag(const char* image, int lane, int c16) {
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(image + tn_read_off(lane, c16, 0)));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(image + tn_read_off(lane, c16, 1)));
  const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return *reinterpret_cast<const bf16x8*>(&v);
}

__global__ __launch_bounds__(256, 2) void gemm_tn_kernel(TnArgs args) {
  // [buffer][operand][image]: 2 x 2 x 2 x 8 KiB
  __shared__ __attribute__((aligned(16))) char lds[2][2][kImages][TN_IMAGE_BYTES];

  // consecutive workgroup ids go round the 8 XCDs: hand each XCD a contiguous run of tiles, so that the N tiles of one row
  // block (which share the A rows) meet in one L2.  The grid is padded to a multiple of 8; surplus workgroups leave as a whole.
  const int per = gridDim.x >> 3;
  const int tile = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
  if (tile >= args.ntiles) return;
  int gi = 0;
  while (gi + 1 < args.ng && tile >= args.g[gi + 1].tile0) ++gi;
  const TnGroup& g = args.g[gi];
  const int local = tile - g.tile0;
  const int m0 = (local / g.ntn) * TN_COLS, n0 = (local % g.ntn) * TN_COLS;
  const int M = g.M, N = g.N, K = g.K;
  const long lda = g.lda, ldb = g.ldb;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ch = tid & 15, r0 = tid >> 4;
  const bool a_ok = m0 + 8 * ch < M, b_ok = n0 + 8 * ch < N;      // the whole 16-byte piece lies below ld (a multiple of 8)
  const bf16_t* ap = g.a + m0 + 8 * ch;
  const bf16_t* bp = g.b + n0 + 8 * ch;
  const int* b_row = g.b_row; const int* b_live = g.b_live;
  const bool do_cs = n0 == 0 && (g.cs0 || g.cs1);

  u32x4 ra[kRowsPerThread], rb[kRowsPerThread];
  // gather tables of the step after the one being loaded: requested with nothing between the requests and consumed one step
  // later, so that no wait for them lands in front of the MFMAs (a wait counts every older load, the tile's included)
  int idx[kRowsPerThread], live[kRowsPerThread];
  auto resolve = [&](int kbase) {
    if (!b_row) return;                            // workgroup-uniform, as is b_live
#pragma unroll
    for (int i = 0; i < kRowsPerThread; ++i) {
      const int k = kbase + r0 + 16 * i, kk = k < K ? k : K - 1;
      idx[i] = b_row[kk];
      live[i] = 1;
    }
    if (b_live) {
#pragma unroll
      for (int i = 0; i < kRowsPerThread; ++i) {
        const int k = kbase + r0 + 16 * i;
        live[i] = b_live[k < K ? k : K - 1];
      }
    }
  };
  auto load = [&](int kbase) {
#pragma unroll
    for (int i = 0; i < kRowsPerThread; ++i) {
      const int k = kbase + r0 + 16 * i;
      int src = k;                                 // source row of B, -1: zeros
      if (b_row) src = live[i] > 0 ? idx[i] : -1;
      ra[i] = u32x4{0u, 0u, 0u, 0u}; rb[i] = u32x4{0u, 0u, 0u, 0u};
      if (a_ok && k < K) ra[i] = *reinterpret_cast<const u32x4*>(ap + k * lda);
      if (b_ok && k < K && src >= 0) rb[i] = *reinterpret_cast<const u32x4*>(bp + src * ldb);
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float cs[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) cs[e] = 0.f;

  const int wm = wave >> 1, wn = wave & 1;
  const int nsteps = (K + kStep - 1) / kStep;
  resolve(0);
  load(0);
  resolve(kStep);
  for (int s = 0; s < nsteps; ++s) {
    char* buf = &lds[s & 1][0][0][0];
#pragma unroll
    for (int i = 0; i < kRowsPerThread; ++i) {
      const int row = r0 + 16 * i;                 // row of the step: image row >> 5, row & 31 inside it
      const int off = (row / TN_BK) * TN_IMAGE_BYTES + tn_store_off(row % TN_BK, ch);
      *reinterpret_cast<u32x4*>(buf + off) = ra[i];
      *reinterpret_cast<u32x4*>(buf + kImages * TN_IMAGE_BYTES + off) = rb[i];
    }
    if (do_cs) {                                   // workgroup-uniform
#pragma unroll
      for (int i = 0; i < kRowsPerThread; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          cs[2 * e] += __uint_as_float(ra[i][e] << 16);
          cs[2 * e + 1] += __uint_as_float(ra[i][e] & 0xffff0000u);
        }
    }
    __syncthreads();
    if (s + 1 < nsteps) {                          // uniform; the loads fly while the MFMAs below run
      load((s + 1) * kStep);
      resolve((s + 2) * kStep);
    }
#pragma unroll
    for (int im = 0; im < kImages; ++im) {
      const char* ia = buf + im * TN_IMAGE_BYTES;
      const char* ib = buf + (kImages + im) * TN_IMAGE_BYTES;
      bf16x8 fa[4], fb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { fa[i] = tr_frag(ia, lane, 4 * wm + i); fb[i] = tr_frag(ib, lane, 4 * wn + i); }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
  }

  // C: lane holds rows 4 * (lane >> 4) + r, column lane & 15 of each 16 x 16 block.  A tile inside C (workgroup-uniform: every
  // tile of the decoder's shapes but the last row block of dW_lin) has no condition per element: the prior values are requested
  // 32 at a time before any is used and the stores follow in one block.  Element by element -- a load, its add and its store
  // behind a branch each -- the memory counter makes every store wait for the one before: 64 dependent round trips per tile.
  float* const cbase = g.c;
  const long ldc = g.ldc;
  const bool accumulate = g.accumulate != 0;
  auto write_c = [&](auto full_tag) {
    constexpr bool kFull = decltype(full_tag)::value;
    float* const cl = cbase + (long)(m0 + 64 * wm + 4 * (lane >> 4)) * ldc + (n0 + 64 * wn + (lane & 15));
#pragma unroll
    for (int i0 = 0; i0 < 4; i0 += 2) {
      float prior[2][4][4];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int m = m0 + 64 * wm + 16 * (i0 + i) + 4 * (lane >> 4) + r, n = n0 + 64 * wn + 16 * j + (lane & 15);
            const bool ok = kFull || (m < M && n < N);
            prior[i][r][j] = 0.f;
            if (accumulate) prior[i][r][j] = ok ? cl[(16 * (i0 + i) + r) * ldc + 16 * j] : 0.f;
          }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int m = m0 + 64 * wm + 16 * (i0 + i) + 4 * (lane >> 4) + r, n = n0 + 64 * wn + 16 * j + (lane & 15);
            if (kFull || (m < M && n < N)) cl[(16 * (i0 + i) + r) * ldc + 16 * j] = prior[i][r][j] + acc[i0 + i][j][r];
          }
    }
  };
  if (m0 + TN_COLS <= M && n0 + TN_COLS <= N) write_c(std::true_type{});
  else write_c(std::false_type{});

  if (do_cs) {
    __syncthreads();                               // every wave is done with the images
    float* red = reinterpret_cast<float*>(&lds[0][0][0][0]);      // [16][128] floats = 8 KiB
#pragma unroll
    for (int e = 0; e < 8; ++e) red[r0 * TN_COLS + 8 * ch + e] = cs[e];
    __syncthreads();
    if (tid < TN_COLS && m0 + tid < M) {
      float sum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) sum += red[r * TN_COLS + tid];
      if (g.cs0) g.cs0[m0 + tid] += sum;
      if (g.cs1) g.cs1[m0 + tid] += sum;
    }
  }
}

}  // namespace

extern "C" int st_gemm_tn_batch(const st_gemm_tn_desc* d, int n, void* stream) {
  ST_CHECK(d && n >= 1 && n <= kMaxGroups, "st_gemm_tn_batch: 1..%d problems per launch", kMaxGroups);
  TnArgs args;
  memset(&args, 0, sizeof(args));
  long tiles = 0;
  for (int i = 0; i < n; ++i) {
    const st_gemm_tn_desc& p = d[i];
    ST_CHECK(p.dtype == ST_BF16, "st_gemm_tn_batch: problem %d: bf16 only (the transposed LDS read is a 16-bit one)", i);
    ST_CHECK(p.a && p.b && p.c, "st_gemm_tn_batch: problem %d: null pointer", i);
    ST_CHECK(p.M >= 1 && p.N >= 1 && p.K >= 1, "st_gemm_tn_batch: problem %d: bad shape M=%d N=%d K=%d", i, p.M, p.N, p.K);
    ST_CHECK(p.lda >= p.M && p.ldb >= p.N && p.ldc >= p.N, "st_gemm_tn_batch: problem %d: leading dimension below the extent (lda=%d M=%d ldb=%d N=%d ldc=%d)",
             i, p.lda, p.M, p.ldb, p.N, p.ldc);
    ST_CHECK(p.lda % 8 == 0 && p.ldb % 8 == 0, "st_gemm_tn_batch: problem %d: lda=%d and ldb=%d must be multiples of 8", i, p.lda, p.ldb);
    ST_CHECK(((reinterpret_cast<uintptr_t>(p.a) | reinterpret_cast<uintptr_t>(p.b)) & 15) == 0, "st_gemm_tn_batch: problem %d: a and b must be 16-byte aligned", i);
    ST_CHECK(!p.b_live || p.b_row, "st_gemm_tn_batch: problem %d: b_live goes with b_row", i);
    TnGroup& g = args.g[i];
    g.a = reinterpret_cast<const bf16_t*>(p.a); g.b = reinterpret_cast<const bf16_t*>(p.b); g.c = p.c;
    g.b_row = p.b_row; g.b_live = p.b_live; g.cs0 = p.colsum0; g.cs1 = p.colsum1;
    g.M = p.M; g.N = p.N; g.K = p.K; g.lda = p.lda; g.ldb = p.ldb; g.ldc = p.ldc; g.accumulate = p.accumulate;
    g.tile0 = (int)tiles;
    g.ntn = (p.N + TN_COLS - 1) / TN_COLS;
    tiles += (long)((p.M + TN_COLS - 1) / TN_COLS) * g.ntn;
    ST_CHECK(tiles < (1L << 24), "st_gemm_tn_batch: too many output tiles");
  }
  args.ng = n; args.ntiles = (int)tiles;
  const int grid = (int)((tiles + 7) / 8 * 8);
  hipLaunchKernelGGL(gemm_tn_kernel, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), args);
  ST_LAUNCH_CHECK();
  return 0;
}
