// Dropout over rows of a packed sequence, outside the recurrence: y[r][c] = keep(row0 + r, c) ? T(float(x[r][c]) * scale) : +0, the
// mask of csrc/dropout.h.  What nn.Dropout does in front of `linear` and on the decoder's inputs (and their gradients) in the recipes the
// reference's decoders are trained with; the inter-layer site of nn.GRU(dropout=p) lives in the cell kernels' epilogues (rnn_kernels.hip).
// One Philox call per 4 consecutive elements; 8- / 16-byte loads and stores; in place allowed (every thread reads its 4 elements
// before it writes them and no other thread touches them; the kernel's pointers are therefore not __restrict__).
#include "common.h"
#include "dropout.h"

namespace {

template <typename T> struct Vec4;
template <> struct Vec4<float> {
  typedef f32x4 type;
  static __device__ __forceinline__ float get(const type& v, int e) { return v[e]; }
  static __device__ __forceinline__ type make(const float* f) { return f32x4{f[0], f[1], f[2], f[3]}; }
};
template <> struct Vec4<bf16_t> {
  typedef u32x2 type;
  static __device__ __forceinline__ float get(const type& v, int e) {
    return __uint_as_float((e & 1) ? (v[e >> 1] & 0xffff0000u) : (v[e >> 1] << 16));
  }
  static __device__ __forceinline__ type make(const float* f) { return u32x2{pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3])}; }
};

template <typename T>
__global__ __launch_bounds__(256) void dropout_rows_kernel(const T* x, T* y, int rows, int cols4, long ldx, long ldy,
                                                           DropKey key, int site, int row0) {
  typedef typename Vec4<T>::type vec_t;
  const long total = (long)rows * cols4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int r = (int)(i / cols4), c4 = (int)(i - (long)r * cols4);
    const vec_t v = *reinterpret_cast<const vec_t*>(x + r * ldx + 4 * c4);
    const DropWords w = drop_words(key, site, row0 + r, c4);
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = w.w[e] >= key.thr ? Vec4<T>::get(v, e) * key.scale : 0.f;
    *reinterpret_cast<vec_t*>(y + r * ldy + 4 * c4) = Vec4<T>::make(o);
  }
}

}  // namespace

// internal launcher (declared in rnn_kernels.h): the entry point below without the argument checks of a public call
int dropout_rows_launch(const void* x, void* y, int dtype, int rows, int cols, int ldx, int ldy, const DropKey& key, int site, int row0,
                        hipStream_t st) {
  if (rows <= 0 || cols <= 0) return 0;
  const long work = (long)rows * (cols / 4);
  long blocks = (work + 255) / 256;
  blocks = blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks);
  if (dtype == ST_BF16)
    hipLaunchKernelGGL(dropout_rows_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, st, (const bf16_t*)x, (bf16_t*)y, rows, cols / 4,
                       (long)ldx, (long)ldy, key, site, row0);
  else
    hipLaunchKernelGGL(dropout_rows_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)x, (float*)y, rows, cols / 4,
                       (long)ldx, (long)ldy, key, site, row0);
  ST_LAUNCH_CHECK();
  return 0;
}

extern "C" int st_dropout_rows(const void* x, void* y, int dtype, int rows, int cols, int ldx, int ldy, double p, long seed, int step,
                               int site, int row0, void* stream) {
  ST_CHECK(x && y, "st_dropout_rows: null pointer");
  ST_CHECK(dtype == ST_F32 || dtype == ST_BF16, "st_dropout_rows: bad dtype %d", dtype);
  ST_CHECK(rows >= 0 && cols >= 0 && cols % 4 == 0, "st_dropout_rows: cols=%d must be a multiple of 4 (rows=%d)", cols, rows);
  ST_CHECK(ldx >= cols && ldy >= cols && ldx % 4 == 0 && ldy % 4 == 0, "st_dropout_rows: ldx=%d and ldy=%d must be multiples of 4 and >= cols=%d",
           ldx, ldy, cols);
  const uintptr_t al = dtype == ST_BF16 ? 8 : 16;   // the kernel moves 4 elements per load / store
  ST_CHECK(reinterpret_cast<uintptr_t>(x) % al == 0 && reinterpret_cast<uintptr_t>(y) % al == 0,
           "st_dropout_rows: x and y must be %d-byte aligned", (int)al);
  ST_CHECK(p >= 0.0 && p < 1.0, "st_dropout_rows: p=%g outside [0, 1)", p);
  ST_CHECK(site >= 0 && site <= kDropSiteInput && row0 >= 0 && step >= 0, "st_dropout_rows: bad site / row0 / step");
  return dropout_rows_launch(x, y, dtype, rows, cols, ldx, ldy, drop_key(p, seed, step), site, row0, reinterpret_cast<hipStream_t>(stream));
}
