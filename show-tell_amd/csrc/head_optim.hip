// Encoder head (Linear -> BatchNorm1d, reference cnn.py:37-38,49) and the optimizers
// (torch.optim.SGD / Adam at main.py:97-100,152) for gfx950.
//
// The head is tiny (B x 2048 x E) and bandwidth-trivial; its GEMMs go through st_conv, the
// BatchNorm1d statistics / gradients use one thread per feature column (coalesced over
// columns, serial over the <= few hundred batch rows).
// The optimizers are single multi-tensor launches over ONE flat fp32 parameter buffer
// (HBM-bound: SGD 3 reads + 2 writes, Adam 4 reads + 3 writes per element, plus the bf16
// shadow copy the MFMA kernels read), instead of torch's per-tensor loops.
#include "decoder_host.h"

namespace {

// BatchNorm1d over [B][E] fp32: a block owns 32 columns, its 8 row groups stride over the batch and meet in LDS
// (128-byte coalesced row segments, E/32 blocks instead of one serial thread per column).
constexpr int kBnTX = 32, kBnTY = 8;
__device__ __forceinline__ float bn1d_colsum(float v, float (*red)[kBnTX]) {
  const int tx = threadIdx.x, ty = threadIdx.y;
  __syncthreads();                      // previous use of red is over
  red[ty][tx] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < kBnTY; ++k) s += red[k][tx];
  return s;
}

template <typename TO>
__global__ __launch_bounds__(256) void bn1d_fwd_kernel(const float* __restrict__ z, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       float* __restrict__ rm, float* __restrict__ rv, float* __restrict__ save_mean,
                                                       float* __restrict__ save_rstd, TO* __restrict__ y, float* __restrict__ y_f32,
                                                       int B, int E, int train, float mom, float eps) {
  __shared__ float red[kBnTY][kBnTX];
  const int e = blockIdx.x * kBnTX + threadIdx.x, ty = threadIdx.y;
  const bool ok = e < E;
  float mean = 0.f, rstd = 0.f;
  if (train) {
    float s = 0.f;
    if (ok) for (int b = ty; b < B; b += kBnTY) s += z[(long)b * E + e];
    mean = bn1d_colsum(s, red) / B;
    float v = 0.f;
    if (ok) for (int b = ty; b < B; b += kBnTY) { const float d = z[(long)b * E + e] - mean; v += d * d; }
    v = bn1d_colsum(v, red);
    const float var = v / B;
    rstd = rsqrtf(var + eps);
    if (ok && ty == 0) {
      const float unb = B > 1 ? v / (B - 1) : var;
      rm[e] = (1.f - mom) * rm[e] + mom * mean;
      rv[e] = (1.f - mom) * rv[e] + mom * unb;
    }
  } else if (ok) {
    mean = rm[e];
    rstd = rsqrtf(rv[e] + eps);
  }
  if (!ok) return;
  if (save_mean && ty == 0) { save_mean[e] = mean; save_rstd[e] = rstd; }
  const float g = gamma[e] * rstd, sh = beta[e] - mean * g;
  for (int b = ty; b < B; b += kBnTY) {
    const float o = z[(long)b * E + e] * g + sh;
    if (y) y[(long)b * E + e] = from_f32<TO>(o);
    if (y_f32) y_f32[(long)b * E + e] = o;
  }
}

template <typename TO>
__global__ __launch_bounds__(256) void bn1d_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ z, const float* __restrict__ gamma,
                                                       const float* __restrict__ save_mean, const float* __restrict__ save_rstd,
                                                       float* __restrict__ dgamma, float* __restrict__ dbeta, TO* __restrict__ dz,
                                                       int B, int E, int ldz, int train) {
  __shared__ float red[kBnTY][kBnTX];
  const int e = blockIdx.x * kBnTX + threadIdx.x, ty = threadIdx.y;
  const bool ok = e < E;
  const float mean = ok ? save_mean[e] : 0.f, rstd = ok ? save_rstd[e] : 0.f, g = ok ? gamma[e] : 0.f;
  float sdy = 0.f, sdyx = 0.f;
  if (ok) for (int b = ty; b < B; b += kBnTY) {
    const float d = dy[(long)b * E + e], xh = (z[(long)b * E + e] - mean) * rstd;
    sdy += d; sdyx += d * xh;
  }
  sdy = bn1d_colsum(sdy, red);
  sdyx = bn1d_colsum(sdyx, red);
  if (!ok) return;
  if (ty == 0) { dgamma[e] += sdyx; dbeta[e] += sdy; }
  const float m1 = sdy / B, m2 = sdyx / B;
  for (int b = ty; b < B; b += kBnTY) {
    const float d = dy[(long)b * E + e], xh = (z[(long)b * E + e] - mean) * rstd;
    const float o = train ? g * rstd * (d - m1 - xh * m2) : g * rstd * d;
    dz[(long)b * ldz + e] = from_f32<TO>(o);
  }
}

__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                  uint16_t* __restrict__ shadow, long n, float lr, float mom, int first, float gscale) {
  for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (long)gridDim.x * blockDim.x * 4) {
    if (i + 3 < n) {
      f32x4 pv = *reinterpret_cast<f32x4*>(p + i);
      const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i);
      f32x4 bv = {0.f, 0.f, 0.f, 0.f};
      if (mom != 0.f && !first) bv = *reinterpret_cast<f32x4*>(buf + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float gg = gv[e] * gscale;
        const float b = (mom != 0.f) ? (first ? gg : mom * bv[e] + gg) : gg;
        bv[e] = b; pv[e] -= lr * b;
      }
      *reinterpret_cast<f32x4*>(p + i) = pv;
      if (mom != 0.f) *reinterpret_cast<f32x4*>(buf + i) = bv;
      if (shadow) *reinterpret_cast<u32x2*>(shadow + i) = u32x2{pack_bf16x2(pv[0], pv[1]), pack_bf16x2(pv[2], pv[3])};
    } else {
      for (long j = i; j < n; ++j) {
        const float gg = g[j] * gscale;
        const float b = (mom != 0.f) ? (first ? gg : mom * buf[j] + gg) : gg;
        if (mom != 0.f) buf[j] = b;
        p[j] -= lr * b;
        if (shadow) shadow[j] = f32_to_bf16_bits(p[j]);
      }
    }
  }
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                   uint16_t* __restrict__ shadow, long n, float lr, float b1, float b2, float eps,
                                                   float bc1, float sqrt_bc2, float gscale) {
  for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (long)gridDim.x * blockDim.x * 4) {
    const int cnt = (i + 3 < n) ? 4 : (int)(n - i);
    for (int e = 0; e < cnt; ++e) {
      const long j = i + e;
      const float gg = g[j] * gscale;
      const float mm = b1 * m[j] + (1.f - b1) * gg;
      const float vv = b2 * v[j] + (1.f - b2) * gg * gg;
      m[j] = mm; v[j] = vv;
      const float denom = sqrtf(vv) / sqrt_bc2 + eps;
      const float np = p[j] - (lr / bc1) * (mm / denom);
      p[j] = np;
      if (shadow) shadow[j] = f32_to_bf16_bits(np);
    }
  }
}

// ---- global-norm clipping, weight decay and the non-finite guard (st_grad_sumsq + st_*_step_ex) -------------------------------
// Two launches: grad_sumsq_kernel leaves one partial sum of squares per block, the kernel boundary makes them visible chip-wide, and
// every block of the step kernel adds them up again in the same fixed order, so that all blocks hold the same bits of the sum
// and take the same side of the finite / non-finite decision.  No float atomics anywhere: same input, same bits.
constexpr int kSumsqMaxParts = 2048;      // the partials buffer the caller owns holds this many floats
constexpr int kOptThreads = 256;

__device__ __forceinline__ float block_sum_256(float v, float* red) {     // wave butterflies, then the four wave sums in wave order
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, long n, float* __restrict__ partials) {
  __shared__ float red[kOptThreads / 64];
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (long)gridDim.x * blockDim.x * 4) {
    if (i + 3 < n) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(g + i);
      a0 += v[0] * v[0]; a1 += v[1] * v[1]; a2 += v[2] * v[2]; a3 += v[3] * v[3];
    } else {
      for (long j = i; j < n; ++j) a0 += g[j] * g[j];
    }
  }
  const float s = block_sum_256((a0 + a1) + (a2 + a3), red);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// The status block (ST_OPTIM_STATUS_WORDS 32-bit words, showtell_hip.h): [0] norm f32, [1] coefficient f32, [2] applied steps,
// [3] skipped steps, [4], [5] the applied count again as two slots: a launch READS slot `parity` in every block and block 0 WRITES
// slot `parity ^ 1` (and the published copy [2]), so no block can see the count this very launch advances; the host alternates parity.
struct ClipHead { float coef; int applied_before; bool skip; };

__device__ __forceinline__ ClipHead clip_head(const float* __restrict__ partials, int nparts, float gscale, float max_norm,
                                              int skip_nonfinite, int parity, int* __restrict__ status, float* red) {
  float s = 0.f;
  for (int k = threadIdx.x; k < nparts; k += kOptThreads) s += partials[k];      // <= 8 per thread, ascending
  s = block_sum_256(s, red);
  const float norm = gscale * sqrtf(s);
  float coef = gscale;
  if (max_norm > 0.f) {
    const float r = max_norm / (norm + 1e-6f);
    coef = gscale * (r > 1.f ? 1.f : r);          // a NaN ratio stays NaN (torch.clamp), unlike fminf
  }
  ClipHead h;
  h.coef = coef;
  h.applied_before = status[4 + parity];
  h.skip = skip_nonfinite && !(fabsf(s) <= 3.402823466e38f);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    reinterpret_cast<float*>(status)[0] = norm;
    reinterpret_cast<float*>(status)[1] = coef;
    const int after = h.applied_before + (h.skip ? 0 : 1);
    status[2] = after; status[4 + (parity ^ 1)] = after;
    if (h.skip) status[3] += 1;
  }
  return h;
}

template <bool WD>
__device__ __forceinline__ void sgd_elem(float& p, float g, float& b, float lr, float mom, int first, float coef, float wd) {
  float gg = g * coef;
  if (WD) gg += wd * p;
  b = (mom != 0.f) ? (first ? gg : mom * b + gg) : gg;
  p -= lr * b;
}

template <bool WD>
__global__ __launch_bounds__(256) void sgd_ex_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                     uint16_t* __restrict__ shadow, long n, float lr, float mom, int first_step, float gscale,
                                                     const float* __restrict__ partials, int nparts, float max_norm, float wd,
                                                     int skip_nonfinite, int parity, int* __restrict__ status) {
  __shared__ float red[kOptThreads / 64];
  const ClipHead h = clip_head(partials, nparts, gscale, max_norm, skip_nonfinite, parity, status, red);
  if (h.skip) return;
  const int first = skip_nonfinite ? h.applied_before == 0 : first_step;     // the first APPLIED step seeds the momentum buffer
  const float coef = h.coef;
  for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (long)gridDim.x * blockDim.x * 4) {
    if (i + 3 < n) {
      f32x4 pv = *reinterpret_cast<f32x4*>(p + i);
      const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i);
      f32x4 bv = {0.f, 0.f, 0.f, 0.f};
      if (mom != 0.f && !first) bv = *reinterpret_cast<f32x4*>(buf + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = pv[e], be = bv[e];
        sgd_elem<WD>(pe, gv[e], be, lr, mom, first, coef, wd);
        pv[e] = pe; bv[e] = be;
      }
      *reinterpret_cast<f32x4*>(p + i) = pv;
      if (mom != 0.f) *reinterpret_cast<f32x4*>(buf + i) = bv;
      if (shadow) *reinterpret_cast<u32x2*>(shadow + i) = u32x2{pack_bf16x2(pv[0], pv[1]), pack_bf16x2(pv[2], pv[3])};
    } else {
      for (long j = i; j < n; ++j) {
        float pj = p[j], b = (mom != 0.f && !first) ? buf[j] : 0.f;
        sgd_elem<WD>(pj, g[j], b, lr, mom, first, coef, wd);
        if (mom != 0.f) buf[j] = b;
        p[j] = pj;
        if (shadow) shadow[j] = f32_to_bf16_bits(pj);
      }
    }
  }
}

// WDM: 0 no decay, 1 L2 (torch.optim.Adam(weight_decay=)), 2 decoupled (torch.optim.AdamW)
template <int WDM>
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float lr, float b1, float b2, float eps, float bc1,
                                          float sqrt_bc2, float coef, float wd) {
  float gg = g * coef;
  if (WDM == 1) gg += wd * p;
  if (WDM == 2) p *= 1.f - lr * wd;
  const float mm = b1 * m + (1.f - b1) * gg;
  const float vv = b2 * v + (1.f - b2) * gg * gg;
  m = mm; v = vv;
  const float denom = sqrtf(vv) / sqrt_bc2 + eps;
  p = p - (lr / bc1) * (mm / denom);
}

template <int WDM>
__global__ __launch_bounds__(256) void adam_ex_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                      uint16_t* __restrict__ shadow, long n, float lr, float b1, float b2, float eps, float bc1_host,
                                                      float sqrt_bc2_host, float gscale, const float* __restrict__ partials, int nparts, float max_norm, float wd,
                                                      int skip_nonfinite, int parity, int* __restrict__ status) {
  __shared__ float red[kOptThreads / 64];
  const ClipHead h = clip_head(partials, nparts, gscale, max_norm, skip_nonfinite, parity, status, red);
  if (h.skip) return;
  // bias correction: the host's, from its step count (the very floats st_adam_step computes: a step that nothing clips or decays
  // keeps its bits), unless steps can be skipped: then from the count of APPLIED steps, which only the device knows
  // (torch: the user skipped optimizer.step())
  float bc1 = bc1_host, sqrt_bc2 = sqrt_bc2_host;
  if (skip_nonfinite) {
    const float t = (float)(h.applied_before + 1);
    bc1 = 1.f - powf(b1, t);
    sqrt_bc2 = sqrtf(1.f - powf(b2, t));
  }
  const float coef = h.coef;
  for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (long)gridDim.x * blockDim.x * 4) {
    if (i + 3 < n) {
      f32x4 pv = *reinterpret_cast<f32x4*>(p + i), mv = *reinterpret_cast<f32x4*>(m + i), vv = *reinterpret_cast<f32x4*>(v + i);
      const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = pv[e], me = mv[e], ve = vv[e];
        adam_elem<WDM>(pe, gv[e], me, ve, lr, b1, b2, eps, bc1, sqrt_bc2, coef, wd);
        pv[e] = pe; mv[e] = me; vv[e] = ve;
      }
      *reinterpret_cast<f32x4*>(p + i) = pv;
      *reinterpret_cast<f32x4*>(m + i) = mv;
      *reinterpret_cast<f32x4*>(v + i) = vv;
      if (shadow) *reinterpret_cast<u32x2*>(shadow + i) = u32x2{pack_bf16x2(pv[0], pv[1]), pack_bf16x2(pv[2], pv[3])};
    } else {
      for (long j = i; j < n; ++j) {
        float pj = p[j], mj = m[j], vj = v[j];
        adam_elem<WDM>(pj, g[j], mj, vj, lr, b1, b2, eps, bc1, sqrt_bc2, coef, wd);
        p[j] = pj; m[j] = mj; v[j] = vj;
        if (shadow) shadow[j] = f32_to_bf16_bits(pj);
      }
    }
  }
}

int optim_grid(long n) {
  long blocks = (n / 4 + 255) / 256; if (blocks < 1) blocks = 1; if (blocks > 2048) blocks = 2048;
  return (int)blocks;
}

}  // namespace

extern "C" size_t st_head_workspace_bytes(int B, int F, int E, int dtype) {
  const size_t es = st_dtype_size(dtype);
  const int Bp = st_up8(B);
  return st_al256((size_t)B * st_up8(E) * es) + st_al256((size_t)E * Bp * es) + st_al256((size_t)F * Bp * es);
}

extern "C" int st_linear_bn1d_forward(const void* x, const void* w, const float* bias, const float* gamma, const float* beta,
                                      float* running_mean, float* running_var, int B, int F, int E, int dtype,
                                      int train, float momentum, float eps,
                                      float* z_out, float* save_mean, float* save_rstd, void* y_dtype, float* y_f32, void* stream) {
  ST_CHECK(x && w && bias && gamma && beta && running_mean && running_var && z_out, "st_linear_bn1d_forward: null pointer");
  ST_CHECK(dtype == ST_F32 || dtype == ST_BF16, "st_linear_bn1d_forward: bad dtype");
  ST_CHECK(B > 0 && F % 8 == 0 && E % 4 == 0, "st_linear_bn1d_forward: need F%%8==0 and E%%4==0 (F=%d E=%d)", F, E);
  ST_CHECK(!train || B > 1, "Expected more than 1 value per channel when training (BatchNorm1d, B=%d)", B);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // B x E output tiles are few (4 at B = 128, E = 512) and K = F is long: 8 K slices in one grouped launch
  const int bk = dtype == ST_BF16 ? 64 : 32;
  const int split = (F % (8 * bk) == 0 && (long)B * E <= 256 * 128 * 64) ? 8 : 0;
  if (st_gemm_nt(x, F, w, F, z_out, E, B, E, F, dtype, ST_F32, bias, stream, 0, split)) return 1;
  const dim3 grid((E + kBnTX - 1) / kBnTX), block(kBnTX, kBnTY);
  if (dtype == ST_BF16)
    hipLaunchKernelGGL(bn1d_fwd_kernel<bf16_t>, grid, block, 0, st, z_out, gamma, beta, running_mean, running_var, save_mean, save_rstd,
                       (bf16_t*)y_dtype, y_f32, B, E, train, momentum, eps);
  else
    hipLaunchKernelGGL(bn1d_fwd_kernel<float>, grid, block, 0, st, z_out, gamma, beta, running_mean, running_var, save_mean, save_rstd,
                       (float*)y_dtype, y_f32, B, E, train, momentum, eps);
  ST_LAUNCH_CHECK();
  return 0;
}

extern "C" int st_linear_bn1d_backward(const float* dy, const float* z, const void* x, const float* gamma,
                                       const float* save_mean, const float* save_rstd, int B, int F, int E, int dtype, int train,
                                       float* dw, float* dbias, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                                       void* stream) {
  ST_CHECK(dy && z && x && gamma && save_mean && save_rstd && dw && dbias && dgamma && dbeta && workspace, "st_linear_bn1d_backward: null pointer");
  ST_CHECK(workspace_bytes >= st_head_workspace_bytes(B, F, E, dtype), "st_linear_bn1d_backward: workspace too small");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const size_t es = st_dtype_size(dtype);
  const int Bp = st_up8(B), Ep = st_up8(E);
  char* ws = reinterpret_cast<char*>(workspace);
  char* dz = ws; ws += st_al256((size_t)B * Ep * es);
  char* dzT = ws; ws += st_al256((size_t)E * Bp * es);
  char* xT = ws;
  const dim3 grid((E + kBnTX - 1) / kBnTX), block(kBnTX, kBnTY);
  if (dtype == ST_BF16)
    hipLaunchKernelGGL(bn1d_bwd_kernel<bf16_t>, grid, block, 0, st, dy, z, gamma, save_mean, save_rstd, dgamma, dbeta, (bf16_t*)dz, B, E, Ep, train);
  else
    hipLaunchKernelGGL(bn1d_bwd_kernel<float>, grid, block, 0, st, dy, z, gamma, save_mean, save_rstd, dgamma, dbeta, (float*)dz, B, E, Ep, train);
  ST_LAUNCH_CHECK();
  // db += colsum(dz) ; dW += dz^T x
  if (st_transpose_colsum(dz, dzT, dbias, dtype, B, E, Ep, Bp, stream)) return 1;
  if (st_transpose(x, xT, dtype, B, F, F, Bp, stream)) return 1;
  return st_gemm_nt(dzT, Bp, xT, Bp, dw, F, E, F, Bp, dtype, ST_F32, nullptr, stream, 1);
}

extern "C" int st_sgd_step(float* param, const float* grad, float* momentum_buf, void* bf16_shadow, long n,
                           float lr, float momentum, int first_step, float grad_scale, void* stream) {
  ST_CHECK(param && grad && (momentum == 0.f || momentum_buf), "st_sgd_step: null pointer");
  if (n <= 0) return 0;
  long blocks = (n / 4 + 255) / 256; if (blocks < 1) blocks = 1; if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(sgd_kernel, dim3((int)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), param, grad, momentum_buf,
                     (uint16_t*)bf16_shadow, n, lr, momentum, first_step, grad_scale);
  ST_LAUNCH_CHECK();
  return 0;
}

extern "C" int st_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* bf16_shadow, long n,
                            float lr, float beta1, float beta2, float eps, int step, float grad_scale, void* stream) {
  ST_CHECK(param && grad && exp_avg && exp_avg_sq && step >= 1, "st_adam_step: bad arguments");
  if (n <= 0) return 0;
  long blocks = (n / 4 + 255) / 256; if (blocks < 1) blocks = 1; if (blocks > 2048) blocks = 2048;
  const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
  hipLaunchKernelGGL(adam_kernel, dim3((int)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), param, grad, exp_avg, exp_avg_sq,
                     (uint16_t*)bf16_shadow, n, lr, beta1, beta2, eps, bc1, sqrtf(bc2), grad_scale);
  ST_LAUNCH_CHECK();
  return 0;
}

extern "C" int st_grad_sumsq_max_parts(void) { return kSumsqMaxParts; }

extern "C" int st_grad_sumsq(const float* grad, long n, float* partials, int* nparts_out, void* stream) {
  ST_CHECK(grad && partials && nparts_out, "st_grad_sumsq: null pointer");
  *nparts_out = 0;
  if (n <= 0) return 0;
  const int blocks = optim_grid(n);       // a function of n alone: the same n always sums in the same order
  static_assert(kSumsqMaxParts >= 2048, "optim_grid's cap must fit the partials buffer");
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(blocks), dim3(kOptThreads), 0, reinterpret_cast<hipStream_t>(stream), grad, n, partials);
  ST_LAUNCH_CHECK();
  *nparts_out = blocks;
  return 0;
}

#define ST_EX_ARGS_CHECK(name)                                                                                        \
  ST_CHECK(partials && status && nparts >= 1 && nparts <= kSumsqMaxParts, name ": need st_grad_sumsq's partials (1..%d of them) and a status block", kSumsqMaxParts); \
  ST_CHECK(parity == 0 || parity == 1, name ": parity must be 0 or 1");                                              \
  ST_CHECK(weight_decay >= 0.f, name ": weight_decay must not be negative")

extern "C" int st_sgd_step_ex(float* param, const float* grad, float* momentum_buf, void* bf16_shadow, long n,
                              float lr, float momentum, int first_step, float grad_scale, const float* partials, int nparts,
                              float max_norm, float weight_decay, int skip_nonfinite, int parity, void* status, void* stream) {
  ST_CHECK(param && grad && (momentum == 0.f || momentum_buf), "st_sgd_step_ex: null pointer");
  if (n <= 0) return 0;
  ST_EX_ARGS_CHECK("st_sgd_step_ex");
  auto kern = weight_decay != 0.f ? sgd_ex_kernel<true> : sgd_ex_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(optim_grid(n)), dim3(kOptThreads), 0, reinterpret_cast<hipStream_t>(stream), param, grad, momentum_buf,
                     (uint16_t*)bf16_shadow, n, lr, momentum, first_step, grad_scale, partials, nparts, max_norm, weight_decay,
                     skip_nonfinite, parity, (int*)status);
  ST_LAUNCH_CHECK();
  return 0;
}

extern "C" int st_adam_step_ex(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* bf16_shadow, long n,
                               float lr, float beta1, float beta2, float eps, int step, float grad_scale, const float* partials,
                               int nparts, float max_norm, float weight_decay, int decoupled, int skip_nonfinite, int parity,
                               void* status, void* stream) {
  ST_CHECK(param && grad && exp_avg && exp_avg_sq && step >= 1, "st_adam_step_ex: bad arguments");
  if (n <= 0) return 0;
  ST_EX_ARGS_CHECK("st_adam_step_ex");
  auto kern = weight_decay == 0.f ? adam_ex_kernel<0> : decoupled ? adam_ex_kernel<2> : adam_ex_kernel<1>;
  const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
  hipLaunchKernelGGL(kern, dim3(optim_grid(n)), dim3(kOptThreads), 0, reinterpret_cast<hipStream_t>(stream), param, grad, exp_avg, exp_avg_sq,
                     (uint16_t*)bf16_shadow, n, lr, beta1, beta2, eps, bc1, sqrtf(bc2), grad_scale, partials, nparts, max_norm, weight_decay,
                     skip_nonfinite, parity, (int*)status);
  ST_LAUNCH_CHECK();
  return 0;
}
