// ResNet-{18,34,50,101,152} encoder forward as one C-ABI call (gfx950).
//
// Replaces `self.model(x)` of the reference encoder (cnn.py:46 / cnn_attn.py:46), i.e.
// torchvision's resnet children()[:-1] / [:-2], and the reshape that follows it
// (cnn.py:48 flatten of the pooled map, cnn_attn.py:49 view(B,2048,49)).
//
// The whole layer sequence is issued from C++ on one stream (no Python per layer, nothing
// allocated or synchronised -> capturable in a hipGraph).  Activations are NHWC in `dtype`.
//   train != 0 : every BatchNorm2d uses batch statistics (main.py:125 calls cnn.train()):
//                conv epilogue accumulates per-channel sum / sum-of-squares, a fused
//                elementwise pass normalises (+residual)(+ReLU) in place, one kernel updates
//                all running buffers at the end.
//   train == 0 : BN is folded to per-channel scale/shift once per call and applied in the
//                conv epilogue together with the residual add and the ReLU.
#include "common.h"
#include <vector>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <string.h>
#include <stdlib.h>

struct ConvL { int cin, cout, k, stride, pad; size_t woff; size_t bnoff; int korder; size_t woff_frag; int ntw; };   // woff_frag: fragment-major copy for st_conv3x3_img (ntw > 0)
struct BlockL { int c1, c2, c3, ds; int stride; };
// The activation-stationary pointwise kernel (one workgroup per 112 rows) takes the 256 -> 1024 conv3 of layer3, the stride-2
// downsample convs of layer2 / layer3 (256 -> 512, 512 -> 1024: many output-channel slices per input row) and layer4's 512 -> 2048
// (49 rows per image: 56 row blocks at B = 128, so the channels are cut into four parts per row block there -- as one workgroup
// per row block it measured 63 us against 32 on st_conv1x1_wreg).  Static per layer: the fragment-major copy is packed for ONE
// kernel's channel permutation (ntw).
static inline bool use_astat(const ConvL& c) {
  if (c.k != 1) return false;
  if (c.stride == 1) return (c.cin == 256 && c.cout == 1024) || (c.cin == 512 && c.cout == 2048);   // conv3 of layer3 / layer4
  return c.stride == 2 && ((c.cin == 256 && c.cout == 512) || (c.cin == 512 && c.cout == 1024));   // downsample convs of layer2 / layer3
}

struct BnTable { int n; int end[160]; float count[160]; int soff[160]; int rep[160]; };   // soff: float offset of the layer's [rep][2C] statistics
struct PendingUpdate { BnTable tab; const float* stats; };

struct st_resnet {
  int version, dtype, bottleneck, cpad0;
  std::vector<ConvL> convs;
  std::vector<BlockL> blocks;
  size_t wtotal = 0, bntotal = 0;
  int feat_dim = 0;
  // train == 2 (statistics now, running buffers later): the layer table of a forward waits here, keyed by its workspace,
  // for st_resnet_update_running -- lets concurrent forwards on different streams apply their momentum updates in order
  mutable std::map<const void*, PendingUpdate> pending;
  mutable std::mutex mu;
  // test / diagnosis aid (st_resnet_set_taps): when set, every forward copies each residual block's OUTPUT ([B][h][w][C], compute
  // dtype) into this buffer, block after block -- the block-by-block parity test feeds them to the oracle one block at a time
  void* taps = nullptr; size_t taps_bytes = 0;
};

namespace {

constexpr int kStatsRepFloats = 8192;   // cap on rep * 2C per layer (what one bn_act block sums in its preamble)

__global__ void bn_update_all_kernel(const float* __restrict__ stats, float* __restrict__ rm, float* __restrict__ rv,
                                     int total, float mom, BnTable t) {
  // stats holds, per layer l with channels [start_l, end_l): rep_l replicas of [sum(C_l) | sumsq(C_l)] at soff_l
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= total) return;
  int l = 0, hi = t.n - 1;                 // first layer whose channel range ends past c (binary search: each probe is a dependent load)
  while (l < hi) {
    const int mid = (l + hi) >> 1;
    if (c >= t.end[mid]) l = mid + 1; else hi = mid;
  }
  const int start = l == 0 ? 0 : t.end[l - 1];
  const int C = t.end[l] - start;
  const float cnt = t.count[l];
  const float* sl = stats + t.soff[l];
  float s = 0.f, ss = 0.f;
  for (int r = 0; r < t.rep[l]; ++r) { s += sl[r * 2 * C + (c - start)]; ss += sl[r * 2 * C + C + (c - start)]; }
  const float mean = s / cnt;
  const float var = fmaxf(ss / cnt - mean * mean, 0.f);
  const float unb = cnt > 1.f ? var * cnt / (cnt - 1.f) : var;
  rm[c] = (1.f - mom) * rm[c] + mom * mean;
  rv[c] = (1.f - mom) * rv[c] + mom * unb;
}

// replica 0 += replicas 1..R-1 of a layer's [R][2C] statistics: one tiny launch after the conv, so that every block of
// the normalise pass reads 2C floats instead of summing R x 2C itself
__global__ void bn_reduce_replicas_kernel(float* __restrict__ stats, int R, int C2) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C2) return;
  // eight replicas per round trip (one dependent load per replica cost the stem's 64-replica reduction 16 us)
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int r = 0;
  for (; r + 8 <= R; r += 8) {
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = stats[(size_t)(r + q) * C2 + i];
#pragma unroll
    for (int q = 0; q < 8; ++q) s[q] += v[q];
  }
  for (; r < R; ++r) s[0] += stats[(size_t)r * C2 + i];
  stats[i] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
}

__global__ void bn_fold_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                               const float* __restrict__ rm, const float* __restrict__ rv,
                               float* __restrict__ scale, float* __restrict__ shift, int total, float eps) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= total) return;
  const float sc = gamma[c] * rsqrtf(rv[c] + eps);
  scale[c] = sc;
  shift[c] = beta[c] - rm[c] * sc;
}

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline int conv_out(int h, int k, int s, int p) { return (h + 2 * p - k) / s + 1; }

}  // namespace

extern "C" int st_resnet_create(int version, int dtype, st_resnet** out) {
  ST_CHECK(out, "st_resnet_create: null out");
  ST_CHECK(dtype == ST_F32 || dtype == ST_BF16, "st_resnet_create: bad dtype %d", dtype);
  int nb[4];
  int bott;
  switch (version) {
    case 18: nb[0] = 2; nb[1] = 2; nb[2] = 2; nb[3] = 2; bott = 0; break;
    case 34: nb[0] = 3; nb[1] = 4; nb[2] = 6; nb[3] = 3; bott = 0; break;
    case 50: nb[0] = 3; nb[1] = 4; nb[2] = 6; nb[3] = 3; bott = 1; break;
    case 101: nb[0] = 3; nb[1] = 4; nb[2] = 23; nb[3] = 3; bott = 1; break;
    case 152: nb[0] = 3; nb[1] = 8; nb[2] = 36; nb[3] = 3; bott = 1; break;
    default:
      // same message as the reference (cnn.py:33)
      st_set_error("Please specify a valid ResNet version. %d doesn't exist.", version);
      return 2;
  }
  st_resnet* r = new (std::nothrow) st_resnet();
  ST_CHECK(r, "st_resnet_create: out of memory");
  r->version = version; r->dtype = dtype; r->bottleneck = bott;
  const int epc = dtype == ST_BF16 ? 8 : 4;
  r->cpad0 = epc;  // 3 input channels zero-padded to one 16-byte chunk
  auto add = [&](int cin, int cout, int k, int s, int p) {
    const int ch = dtype == ST_BF16 ? 64 : 32;
    ConvL c{cin, cout, k, s, p, r->wtotal, r->bntotal, (k > 1 && cin % ch == 0) ? 1 : 0, 0, 0};
    const int cin_p = (cin == 3) ? r->cpad0 : cin;
    r->wtotal += (size_t)cout * k * k * cin_p;
    // 3x3 stride-1 layers get a second, fragment-major copy of their filters for the image-resident kernel (bf16 only);
    // which kernel runs is decided per call from the map size (224 x 224 is nominal: 8 x 8 asks "is there a kernel at all")
    if (dtype == ST_BF16 && k == 3 && s == 1 && p == 1) {
      c.ntw = st_conv3x3_img_supported(8, 8, cin, cout);
      if (c.ntw > 0) { c.woff_frag = r->wtotal; r->wtotal += (size_t)cout * 9 * cin; }
    }
    // the stride-2 3x3 convs of the bottleneck nets (conv2 of the first block of layer2 / 3 / 4): K-streaming kernel, fragment-major copy
    if (dtype == ST_BF16 && k == 3 && s == 2 && p == 1) {
      c.ntw = st_conv3x3_s2_supported(cin, cout);
      if (c.ntw > 0) { c.woff_frag = r->wtotal; r->wtotal += (size_t)cout * 9 * cin; }
    }
    // pointwise layers with <= 512 input channels: fragment-major copy for the register-resident-filter kernel (st_conv1x1_wreg);
    // a stride-2 512-channel layer the activation-stationary kernel does not take stays with st_conv (measured slower on wreg)
    if (dtype == ST_BF16 && k == 1 && p == 0 && (use_astat(c) || !(s == 2 && cin == 512))) {
      c.ntw = use_astat(c) ? st_conv1x1_astat_supported(cin, cout) : 0;    // conv3 of layer3, downsample of layer2 / layer3
      if (c.ntw == 0) c.ntw = st_conv1x1_wreg_supported(cin, cout);
      if (c.ntw == 0) c.ntw = st_conv1x1_kstream_supported(cin, cout);     // 1024 / 2048 input channels: the K-streaming kernel
      if (c.ntw > 0) { c.woff_frag = r->wtotal; r->wtotal += (size_t)cout * cin; }
    }
    r->bntotal += cout;
    r->convs.push_back(c);
    return (int)r->convs.size() - 1;
  };
  add(3, 64, 7, 2, 3);
  int inpl = 64;
  const int planes[4] = {64, 128, 256, 512};
  const int exp = bott ? 4 : 1;
  for (int li = 0; li < 4; ++li)
    for (int bi = 0; bi < nb[li]; ++bi) {
      const int s = bi == 0 ? (li == 0 ? 1 : 2) : 1;
      BlockL b; b.stride = s; b.c3 = -1; b.ds = -1;
      if (bott) {
        b.c1 = add(inpl, planes[li], 1, 1, 0);
        b.c2 = add(planes[li], planes[li], 3, s, 1);
        b.c3 = add(planes[li], planes[li] * 4, 1, 1, 0);
      } else {
        b.c1 = add(inpl, planes[li], 3, s, 1);
        b.c2 = add(planes[li], planes[li], 3, 1, 1);
      }
      if (bi == 0 && (s != 1 || inpl != planes[li] * exp)) b.ds = add(inpl, planes[li] * exp, 1, s, 0);
      inpl = planes[li] * exp;
      r->blocks.push_back(b);
    }
  r->feat_dim = inpl;
  ST_CHECK(r->convs.size() <= 160, "st_resnet_create: too many layers");
  *out = r;
  return 0;
}

extern "C" void st_resnet_destroy(st_resnet* r) { delete r; }
extern "C" int st_resnet_num_convs(const st_resnet* r) { return r ? (int)r->convs.size() : -1; }
extern "C" int st_resnet_feat_dim(const st_resnet* r) { return r ? r->feat_dim : -1; }
extern "C" size_t st_resnet_weight_elems(const st_resnet* r) { return r ? r->wtotal : 0; }
extern "C" size_t st_resnet_bn_channels(const st_resnet* r) { return r ? r->bntotal : 0; }

extern "C" int st_resnet_conv_info(const st_resnet* r, int i, int* cin, int* cout, int* k, int* stride, int* pad,
                                   int* cin_padded, size_t* weight_offset, size_t* bn_offset, int* k_order,
                                   size_t* frag_weight_offset, int* frag_ntw) {
  ST_CHECK(r && i >= 0 && i < (int)r->convs.size(), "st_resnet_conv_info: bad index %d", i);
  const ConvL& c = r->convs[i];
  if (cin) *cin = c.cin;
  if (cout) *cout = c.cout;
  if (k) *k = c.k;
  if (stride) *stride = c.stride;
  if (pad) *pad = c.pad;
  if (cin_padded) *cin_padded = c.cin == 3 ? r->cpad0 : c.cin;
  if (weight_offset) *weight_offset = c.woff;
  if (bn_offset) *bn_offset = c.bnoff;
  if (k_order) *k_order = c.korder;
  if (frag_weight_offset) *frag_weight_offset = c.woff_frag;
  if (frag_ntw) *frag_ntw = c.ntw;
  return 0;
}

extern "C" int st_resnet_set_taps(st_resnet* r, void* buf, size_t bytes) {
  ST_CHECK(r && (buf || bytes == 0), "st_resnet_set_taps: null pointer");
  std::lock_guard<std::mutex> lk(r->mu);
  r->taps = buf; r->taps_bytes = buf ? bytes : 0;
  return 0;
}

namespace {
// ST_LAYER_LOG=<file>: one line per kernel launch of a forward, in launch order -- which kernel family took which layer, its
// geometry, algorithmic FLOPs and HBM bytes, statistics replicas written / read (tools/layer_table.py joins it with the rocprofv3
// kernel trace of the same process).  The same lines as st_resnet_plan.
FILE* layer_log() {
  static FILE* f = [] { const char* e = getenv("ST_LAYER_LOG"); return e && *e ? fopen(e, "w") : nullptr; }();
  return f;
}
struct Layout { size_t in_bytes, s2dw_bytes, stem_bytes, wide_bytes, narrow_bytes, stats_bytes, fold_bytes, total; };
// Space-to-depth stem (even H, W): the 7x7 stride-2 pad-3 conv over 3 channels is the same sum as a 4x4 stride-1
// conv over the 2x2-blocked image (12 channels, padded to 16; 2 zero rows/cols before, 1 after).  Four neighbouring
// blocked pixels are 128 contiguous bytes, so each filter row is one whole-line tap of the fast loader
// (st_conv sliding-window form) instead of 49 scattered 16-byte gathers per output pixel.
inline bool stem_s2d(int H, int W) { return H % 2 == 0 && W % 2 == 0; }
Layout make_layout(const st_resnet* r, int B, int H, int W) {
  const size_t es = st_dtype_size(r->dtype);
  Layout p;
  p.in_bytes = align256((size_t)B * H * W * r->cpad0 * es);
  if (stem_s2d(H, W)) { const size_t b2 = align256((size_t)B * (H / 2 + 3) * (W / 2 + 3) * 16 * es); if (b2 > p.in_bytes) p.in_bytes = b2; }
  p.s2dw_bytes = align256((size_t)64 * 256 * es);
  const int h1 = conv_out(H, 7, 2, 3), w1 = conv_out(W, 7, 2, 3);
  p.stem_bytes = align256((size_t)B * h1 * w1 * 64 * es);
  const int h2 = conv_out(h1, 3, 2, 1), w2 = conv_out(w1, 3, 2, 1);
  // widest block tensors live at layer1 resolution
  const size_t wide_c = r->bottleneck ? 256 : 64;
  p.wide_bytes = align256((size_t)B * h2 * w2 * wide_c * es);
  p.narrow_bytes = align256((size_t)B * h2 * w2 * 128 * es);  // >= any conv1/conv2 output (layer2 conv1 at layer1 res: 128 ch)
  p.stats_bytes = align256((2 * r->bntotal + (size_t)kStatsRepFloats * r->convs.size()) * sizeof(float));
  p.fold_bytes = align256(2 * r->bntotal * sizeof(float));
  p.total = p.in_bytes + p.s2dw_bytes + p.stem_bytes + 3 * p.wide_bytes + 2 * p.narrow_bytes + p.stats_bytes + p.fold_bytes;
  return p;
}

// A forward is planned on the host first (plan_forward: every kernel choice, replica count and workspace slot), then the
// executor (st_resnet_forward) fills one descriptor per entry and launches it.
enum Route {
  R_IGEMM, R_IMG, R_S2, R_WREG, R_ASTAT, R_KSTREAM,   // one conv on st_conv / st_conv3x3_img / st_conv3x3_s2 / the pointwise kernels
  R_KFUSE, R_B2B, R_B2B0, R_C3C1,                     // the previous block's end fused into this conv1 (b2b N = 0: no conv1)
  R_STEM, R_STEM_POOL, R_MAXPOOL,                     // generic stem conv (st_conv), its pool; the fused bf16 stem
  R_BN_ACT, R_REDUCE, R_TAP                           // normalise pass, statistics replicas -> replica 0, st_resnet_set_taps copy
};
// workspace slots: input, stem output, wide[3] (block inputs / outputs), narrow[2] (conv1 / conv2 outputs)
enum Slot { S_NONE = -1, S_IN, S_STEM, S_WIDE, S_NARROW = S_WIDE + 3, S_COUNT = S_NARROW + 2 };

struct Launch {
  Route route;
  int ci;               // the conv (bn_act / reduce: whose statistics; tap: whose output; kfuse / b2b / c3c1: the next conv1)
  int hin, win;         // input map (bn_act / tap: the tensor's map)
  int x, y, res, xout;  // slots: input (b2b / c3c1: raw conv2 output), output (S_NONE: statistics only), identity or eval
                        // residual, block output formed on the way (kfuse / b2b / c3c1)
  int relu;             // eval epilogue
  int in_ci;            // conv whose BatchNorm (+ ReLU) the loader applies (kfuse: the previous conv3; b2b / c3c1: its bn2)
  int pc;               // kfuse / b2b / c3c1: the previous block's conv3 (b2b N = 0: this block's)
  int id_ci;            // the identity's BatchNorm source (a downsample conv), -1: none
  int rep_out, rep_in;  // statistics replicas written / read (reduce: summed)
};
constexpr int kMaxLaunches = 768;   // >= 8 + 14 per block (ResNet-152: 50 blocks)
struct FwdPlan { int n; bool s2d; int h, w, out; BnTable tab; Launch l[kMaxLaunches]; };

int plan_forward(const st_resnet* r, int B, int H, int W, bool train, FwdPlan& p) {
  const int nconv = (int)r->convs.size(), nblk = (int)r->blocks.size();
  ST_CHECK(nconv <= 160 && 8 + 14 * nblk <= kMaxLaunches, "st_resnet_forward: too many layers");
  const bool bf16 = r->dtype == ST_BF16;
  BnTable& tab = p.tab;
  tab.n = nconv;
  for (int i = 0; i < nconv; ++i) { tab.end[i] = (int)(r->convs[i].bnoff + r->convs[i].cout); tab.count[i] = 1.f; tab.soff[i] = 0; tab.rep[i] = 1; }
  // pass 1: every conv's input map and the kernel it runs on by itself (res: eval epilogue with a residual)
  int hin[160], win[160], hout[160], wout[160];
  Route rt[160];
  auto geo = [&](int ci, int h, int w, bool res) {
    const ConvL& c = r->convs[ci];
    hin[ci] = h; win[ci] = w;
    hout[ci] = conv_out(h, c.k, c.stride, c.pad); wout[ci] = conv_out(w, c.k, c.stride, c.pad);
    tab.count[ci] = (float)((long)B * hout[ci] * wout[ci]);
    // (eval mode: conv3 takes the block's identity in its epilogue -- the register-filter and activation-stationary kernels have that
    // form for stride 1 and <= 512 input channels, i.e. every conv3 of a Bottleneck; the 3x3 kernels do not have it)
    rt[ci] = R_IGEMM;
    if (!bf16 || c.ntw == 0) return;
    if (c.k == 1 && (!res || (c.stride == 1 && c.cin <= 512))) rt[ci] = use_astat(c) ? R_ASTAT : c.cin > 512 ? R_KSTREAM : R_WREG;
    else if (c.k == 3 && c.stride == 1 && !res && st_conv3x3_img_supported(h, w, c.cin, c.cout) == c.ntw) rt[ci] = R_IMG;
    else if (c.k == 3 && c.stride == 2 && !res && st_conv3x3_s2_supported(c.cin, c.cout) == c.ntw && (long)B * h * w * c.cin * 2 < (1L << 31))
      rt[ci] = R_S2;
  };
  geo(0, H, W, false);
  rt[0] = R_STEM;
  int h = conv_out(hout[0], 3, 2, 1), w = conv_out(wout[0], 3, 2, 1);
  for (const BlockL& b : r->blocks) {
    geo(b.c1, h, w, false);
    if (b.ds >= 0) geo(b.ds, h, w, false);
    if (r->bottleneck) { geo(b.c2, hout[b.c1], wout[b.c1], false); geo(b.c3, hout[b.c2], wout[b.c2], !train); }
    else geo(b.c2, hout[b.c1], wout[b.c1], !train);
    h = hout[r->bottleneck ? b.c3 : b.c2]; w = wout[r->bottleneck ? b.c3 : b.c2];
  }
  p.h = h; p.w = w;

  // pass 2: the launches.  rep_in is read when the consumer is added, so it is final: a producer's reduction runs right behind it.
  p.n = 0;
  int stats_used = 0;   // floats handed out so far
  auto add = [&](Route k, int ci, int x, int y, int in_ci) -> Launch& {
    Launch& l = p.l[p.n++];
    l = Launch{k, ci, hin[ci], win[ci], x, y, S_NONE, S_NONE, 1, in_ci, -1, -1, 0, in_ci >= 0 ? tab.rep[in_ci] : 0};
    return l;
  };
  // train: the conv's kernel writes rep_out replicas of its statistics.  Every consumer sums up to 16 replicas itself (bn_act, the
  // conv_img.hip / b2b / c3c1 loaders, the running-buffer update) except igemm's input transform and the stem's pool (rep0): those
  // read replica 0, behind a reduction launch
  auto produce = [&](Launch& l, bool rep0) {
    if (!train) return;
    const ConvL& c = r->convs[l.ci];
    const auto fits = [&](int rep) { return rep * 2 * c.cout <= kStatsRepFloats; };
    int rep = 1;
    if (l.route == R_IGEMM || l.route == R_STEM) {
      // keep ~128-256 pixel tiles per replica (same-address atomics serialise)
      const long tiles = ((long)B * hout[l.ci] * wout[l.ci] + 127) / 128;
      while (rep < 64 && tiles / (rep * 2) >= 128 && fits(rep * 2)) rep *= 2;
    } else if (l.route == R_IMG) {
      const long items = (long)B * ((l.hin * (l.win + 2) + 223) / 224);   // ~ workgroups along M
      while (rep < 4 && items / (rep * 2) >= 4 && fits(rep * 2)) rep *= 2;
    } else {
      // four replicas: the statistics leave a workgroup as full-wave atomics over consecutive channels (block_stats_flush), so the
      // same-address queue is what is left to spread -- and every consumer adds the replicas up in its prologue (cheap at 4)
      while (rep < 4 && fits(rep * 2)) rep *= 2;
    }
    tab.soff[l.ci] = stats_used; tab.rep[l.ci] = l.rep_out = rep;
    stats_used += rep * 2 * c.cout;
    if (rep > 1 && (rep0 || rep > 16)) {
      Launch& q = add(R_REDUCE, l.ci, S_NONE, S_NONE, -1);
      q.rep_out = 1; q.rep_in = rep;
      tab.rep[l.ci] = 1;
    }
  };
  auto bnact = [&](int ci, int x, int res, int id_ci) {      // train-mode normalise (+identity [+its BN]) + ReLU, in place
    Launch& l = add(R_BN_ACT, ci, x, x, ci);
    l.hin = hout[ci]; l.win = wout[ci]; l.res = res; l.id_ci = id_ci;
  };
  auto tap = [&](int ci, int slot) { Launch& l = add(R_TAP, ci, slot, S_NONE, -1); l.hin = hout[ci]; l.win = wout[ci]; };

  // bf16 bottleneck nets on even image sizes: the whole stem (conv1 + statistics + maxpool) is ONE kernel (conv_stem.hip).  In train
  // mode it leaves the pooled RAW conv output in wide[0]; bn1 + relu are applied by the loaders of its two consumers (conv1 and the
  // downsample conv of the first block, both on st_conv1x1_wreg: they sum the 8 replicas) -- pooling commutes with the monotone
  // per-channel map, see conv_stem.hip.
  p.s2d = stem_s2d(H, W);
  const BlockL* b0 = nblk ? &r->blocks[0] : nullptr;
  const bool stem_fused = p.s2d && r->bottleneck && b0 && b0->ds >= 0 && rt[b0->c1] == R_WREG && rt[b0->ds] == R_WREG;
  if (stem_fused) {
    Launch& l = add(R_STEM_POOL, 0, S_IN, S_WIDE, -1);
    if (train) { tab.soff[0] = stats_used; tab.rep[0] = l.rep_out = 8; stats_used += 8 * 2 * r->convs[0].cout; }
  } else {
    produce(add(R_STEM, 0, S_IN, S_STEM, -1), true);
    Launch& l = add(R_MAXPOOL, 0, S_STEM, S_WIDE, train ? 0 : -1);   // train: bn1 + relu folded into the pool
    l.hin = hout[0]; l.win = wout[0];
  }
  const int stem_in = (stem_fused && train) ? 0 : -1;   // the first block's conv1 / downsample read relu(bn1(.)) of wide[0] in their loaders

  // a block whose end the NEXT block's conv1 launch forms (kfuse / b2b / c3c1): wide[raw] holds its raw conv3 output (b2b / c3c1:
  // never written), wide[res] its identity
  struct Pending { bool on; Route k; int pc, c2, id_ci, raw, res; } pend{false, R_KFUSE, -1, -1, -1, 0, 0};
  int cur = 0;  // wide[cur] holds the block input
  for (int bi = 0; bi < nblk; ++bi) {
    const BlockL& b = r->blocks[bi];
    int x1 = S_WIDE + cur;
    if (pend.on) {   // the buffer that is neither the raw conv3 output nor the identity takes x (b2b / c3c1: conv3's buffer)
      x1 = pend.k == R_KFUSE ? S_WIDE + pend.raw : S_NARROW + 1;
      cur = pend.k == R_KFUSE ? 3 - pend.raw - pend.res : pend.raw;
    }
    const int xin = S_WIDE + cur, oth = (cur + 1) % 3, dsb = (cur + 2) % 3;
    const int res = b.ds >= 0 ? S_WIDE + dsb : xin;
    const int in0 = bi == 0 ? stem_in : -1;
    const ConvL& c2 = r->convs[b.c2];
    if (r->bottleneck) {
      const ConvL& c3 = r->convs[b.c3];
      // train: bn1 + relu ride in conv2's loader -- the image-resident and stride-2 kernels sum conv1's replicas, st_conv (igemm
      // MODE 2, padding taps stay zero) reads replica 0 behind a reduction (5 us against a 14 - 44 us pass over the tensor)
      const bool in1 = train && bf16 && (rt[b.c2] == R_IMG || c2.cin % 64 == 0);
      // train: bn2 + relu ride in conv3's loader; needs whole 64-channel (f32: 32) K tiles, which every bottleneck width satisfies
      const bool in2 = train && c3.cin % 64 == 0;
      // 14 x 14 blocks (256 -> 1024 -> next conv1 1024 -> 256) and 28 x 28 blocks (128 -> 512 -> 128), train AND eval: conv3 + block
      // end + next conv1 as one kernel (st_conv_c3c1).  Train: conv3 runs here as a statistics-only pass (y == NULL); an identity that
      // still needs its own BatchNorm (the block behind a downsample conv) rides in the kernel's IDBN form.  Eval: conv3 is not
      // launched at all.  The kernel indexes both fragment-major filter copies with fixed tile permutations: conv3 packed with
      // ntw = 2, conv1 with N / 64 (as st_conv_b2b, conv_b2b.hip:63-65: a retuned pw_cfg table / ST_PW_CFG must not reach them).
      const ConvL* n1 = bi + 1 < nblk ? &r->convs[r->blocks[bi + 1].c1] : nullptr;
      const bool c3c1 = n1 && c3.ntw == 2 && n1->ntw == n1->cout / 64 && st_conv_c3c1_supported(c3.cin, c3.cout, n1->cout) &&
                        (!train || in2) && (long)B * hout[b.c2] * wout[b.c2] * c3.cout * 2 < (1L << 31);
      // Train, 256-channel block inputs (layer1 and the first block of layer2): the block-end pass relu(bn3(raw) + identity) is formed
      // by the NEXT block's conv1 loader (st_conv1x1_kfuse) -- that pass and conv1 are both HBM time there and the fusion drops one full
      // read of the widest tensor (measured 168 -> 125 us per transition at 56 x 56, B = 128).  Wider inputs stay separate: their conv1
      // needs several channel slices per row (each would re-read both inputs) or, at 1024 channels, is MFMA-bound (measured slower fused).
      const bool kfuse = n1 && !c3c1 && train && rt[r->blocks[bi + 1].c1] == R_WREG && n1->cin == 256 &&
                         st_conv1x1_kfuse_supported(n1->cin, n1->cout) == n1->ntw;
      // conv3 recomputed inside st_conv_b2b, run here for its statistics only: at the 56 x 56 boundaries with the next conv1 (64 -> 256
      // -> 64 / 128), at 28 x 28 (128 -> 512, N = 0) stopping at the block output x = relu(bn3(conv3(..)) + identity) -- the raw
      // 512-channel tensor (103 MB at B = 128) is neither written nor read
      const bool b2b = !c3c1 && in2 && rt[b.c3] == R_WREG && c3.ntw == 2 && (!kfuse || n1->ntw == n1->cout / 64) &&
                       st_conv_b2b_supported(c3.cin, c3.cout, kfuse ? n1->cout : 0);

      Launch& l1 = add(pend.on ? pend.k : rt[b.c1], b.c1, x1, S_NARROW, pend.on ? (pend.k == R_KFUSE ? pend.pc : train ? pend.c2 : -1) : in0);
      if (pend.on) { l1.pc = pend.pc; l1.res = S_WIDE + pend.res; l1.id_ci = pend.id_ci; l1.xout = xin; }
      produce(l1, in1 && rt[b.c2] == R_IGEMM);
      if (pend.on) tap(pend.pc, xin);      // the PREVIOUS block's output was formed by this conv1's loader
      if (train && !in1) bnact(b.c1, S_NARROW, S_NONE, -1);
      produce(add(rt[b.c2], b.c2, S_NARROW, S_NARROW + 1, in1 ? b.c1 : -1), in2 && rt[b.c3] == R_IGEMM);
      if (train && !in2) bnact(b.c2, S_NARROW + 1, S_NONE, -1);
      if (b.ds >= 0) { Launch& d = add(rt[b.ds], b.ds, xin, res, in0); d.relu = 0; produce(d, false); }
      if (train || !c3c1) {
        Launch& l3 = add(rt[b.c3], b.c3, S_NARROW + 1, (c3c1 || b2b) ? S_NONE : S_WIDE + oth, in2 ? b.c2 : -1);
        l3.res = train ? S_NONE : res;
        produce(l3, false);
      }
      pend = Pending{c3c1 || kfuse, c3c1 ? R_C3C1 : b2b ? R_B2B : R_KFUSE, b.c3, b.c2, b.ds, oth, b.ds >= 0 ? dsb : cur};
      if (b2b && !kfuse) {
        Launch& l = add(R_B2B0, b.c3, S_NARROW + 1, S_NONE, b.c2);
        l.pc = b.c3; l.res = res; l.id_ci = b.ds; l.xout = S_WIDE + oth;
      } else if (train && !pend.on) bnact(b.c3, S_WIDE + oth, res, b.ds);
    } else {
      const bool in1 = train && rt[b.c2] == R_IMG;   // bn1 + relu ride in conv2's fill
      produce(add(rt[b.c1], b.c1, xin, S_NARROW, -1), false);
      if (train && !in1) bnact(b.c1, S_NARROW, S_NONE, -1);
      if (b.ds >= 0) { Launch& d = add(rt[b.ds], b.ds, xin, res, -1); d.relu = 0; produce(d, false); }
      Launch& l2 = add(rt[b.c2], b.c2, S_NARROW, S_WIDE + oth, in1 ? b.c1 : -1);
      l2.res = train ? S_NONE : res;
      produce(l2, false);
      if (train) bnact(b.c2, S_WIDE + oth, res, b.ds);
    }
    cur = oth;
    if (!pend.on) tap(r->bottleneck ? b.c3 : b.c2, S_WIDE + cur);
  }
  p.out = S_WIDE + cur;
  return 0;
}

// The ST_LAYER_LOG / st_resnet_plan line of a launch (0: a launch that is not logged)
int format_launch(const st_resnet* r, int B, const Launch& l, char* buf, size_t n) {
  const ConvL& c = r->convs[l.ci];
  const ConvL& pc = r->convs[l.pc >= 0 ? l.pc : l.ci];
  const double es = (double)st_dtype_size(r->dtype), rows = (double)B * l.hin * l.win;
  const double rows_o = (double)B * conv_out(l.hin, c.k, c.stride, c.pad) * conv_out(l.win, c.k, c.stride, c.pad);
  const char *fam = "", *what = "";
  int cin = c.cin, cout = c.cout, k = c.k, stride = c.stride, hin = l.hin, win = l.win;
  double fl = 0.0, by = 0.0;
  switch (l.route) {
    case R_STEM: case R_IGEMM: {
      const int cin_p = c.cin == 3 ? r->cpad0 : c.cin;
      fam = "igemm"; what = l.res != S_NONE ? "conv + residual (eval)" : "conv";
      fl = 2.0 * rows_o * c.k * c.k * c.cin * c.cout;
      by = (rows * cin_p + (double)c.k * c.k * cin_p * c.cout + rows_o * c.cout * (l.res != S_NONE ? 2.0 : 1.0)) * es;
      break;
    }
    case R_WREG: case R_ASTAT: case R_KSTREAM:
      fam = l.route == R_WREG ? "conv1x1_wreg" : l.route == R_ASTAT ? "conv1x1_astat" : "conv1x1_kstream";
      what = l.route == R_WREG && l.y == S_NONE ? "1x1 statistics only" : "1x1";
      fl = 2.0 * rows_o * c.cin * c.cout;
      by = (rows_o * c.cin + (double)c.cin * c.cout + (l.y != S_NONE ? rows_o * c.cout * (l.res != S_NONE ? 2.0 : 1.0) : 0.0)) * es; break;
    case R_IMG:
      fam = "conv3x3_img"; what = "3x3"; fl = 2.0 * rows * 9.0 * c.cin * c.cout; by = (rows * (c.cin + c.cout) + 9.0 * c.cin * c.cout) * es; break;
    case R_S2:
      fam = "conv3x3_s2"; what = "3x3 stride 2"; fl = 2.0 * rows_o * 9.0 * c.cin * c.cout;
      by = (rows * c.cin + rows_o * c.cout + 9.0 * c.cin * c.cout) * es; break;
    case R_KFUSE:
      fam = "conv1x1_wreg"; what = "block end (bn3 + identity + relu) fused into conv1";
      fl = 2.0 * rows * c.cin * c.cout; by = rows * (3.0 * c.cin + c.cout) * es; break;
    case R_B2B:
      fam = "conv_b2b"; what = "conv3 recomputed + bn3 + identity + relu + next conv1"; cin = pc.cin;
      fl = 2.0 * rows * ((double)pc.cin * pc.cout + (double)c.cin * c.cout); by = rows * (pc.cin + 2.0 * pc.cout + c.cout) * es; break;
    case R_B2B0:
      fam = "conv_b2b"; what = "conv3 recomputed + bn3 + identity + relu";
      fl = 2.0 * rows * c.cin * c.cout; by = rows * (c.cin + 2.0 * c.cout) * es; break;
    case R_C3C1:
      fam = "conv_c3c1"; what = "conv3 + block end (bn3 + identity + relu) + next conv1"; cin = pc.cin;
      fl = 2.0 * rows * ((double)pc.cin * pc.cout + (double)c.cin * c.cout);
      by = (rows * (pc.cin + 2.0 * pc.cout + c.cout) + (double)pc.cin * pc.cout + (double)c.cin * c.cout) * es; break;
    case R_STEM_POOL: {
      const int h = conv_out(l.hin, 7, 2, 3), w = conv_out(l.win, 7, 2, 3);
      fam = "stem_pool"; what = "7x7/2 conv + statistics + 3x3/2 pool";
      fl = 2.0 * B * h * w * 147.0 * 64;
      by = (double)B * (l.hin / 2 + 3) * (l.win / 2 + 3) * 16 * es + (double)B * conv_out(h, 3, 2, 1) * conv_out(w, 3, 2, 1) * 64 * es;
      break;
    }
    case R_BN_ACT:
      fam = "bn_act"; what = l.res != S_NONE ? "bn + identity + relu" : "bn + relu"; cin = c.cout; k = stride = hin = win = 0;
      by = rows * c.cout * (l.res != S_NONE ? 3.0 : 2.0) * es; break;
    case R_REDUCE:
      fam = "bn_reduce_replicas"; what = "statistics replicas -> replica 0"; cin = c.cout; k = stride = hin = win = 0; break;
    default: return 0;
  }
  return snprintf(buf, n, "%s,%s,%d,%d,%d,%d,%d,%d,%.0f,%.0f,%d,%d\n", fam, what, cin, cout, k, stride, hin, win, fl, by, l.rep_out, l.rep_in);
}
}  // namespace

extern "C" size_t st_resnet_workspace_bytes(const st_resnet* r, int B, int H, int W) {
  if (!r || B <= 0 || H < 32 || W < 32) return 0;
  return make_layout(r, B, H, W).total;
}

extern "C" int st_resnet_plan(const st_resnet* r, int B, int H, int W, int train, char* buf, size_t bytes) {
  if (!r || B <= 0 || H < 32 || W < 32) { st_set_error("st_resnet_plan: bad arguments"); return -1; }
  FwdPlan p;
  if (plan_forward(r, B, H, W, train != 0, p)) return -1;
  std::string text;
  char line[256];
  for (int i = 0; i < p.n; ++i) text.append(line, format_launch(r, B, p.l[i], line, sizeof(line)));
  if (buf && bytes > text.size()) memcpy(buf, text.c_str(), text.size() + 1);
  return (int)text.size();
}

extern "C" int st_resnet_forward(const st_resnet* r, const float* images_nchw, int B, int H, int W,
                                 const void* weights, const float* bn_gamma, const float* bn_beta,
                                 float* bn_running_mean, float* bn_running_var,
                                 int train, float momentum, float eps,
                                 void* workspace, size_t workspace_bytes,
                                 void* feat_nhwc_out, void* pooled_out, int pooled_dtype, float* ncp_out,
                                 void* stream) {
  ST_CHECK(r && images_nchw && weights && bn_gamma && bn_beta && bn_running_mean && bn_running_var && workspace,
           "st_resnet_forward: null pointer");
  ST_CHECK(B > 0 && H >= 32 && W >= 32, "st_resnet_forward: bad input size %dx%dx%d", B, H, W);
  const Layout lay = make_layout(r, B, H, W);
  ST_CHECK(workspace_bytes >= lay.total, "st_resnet_forward: workspace too small (%zu < %zu)", workspace_bytes, lay.total);
  FwdPlan p;
  if (plan_forward(r, B, H, W, train != 0, p)) return 1;
  const BnTable& tab = p.tab;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int dt = r->dtype;
  const size_t es = st_dtype_size(dt);
  char* ws = reinterpret_cast<char*>(workspace);
  char* slot[S_COUNT];
  slot[S_IN] = ws; ws += lay.in_bytes;
  char* s2dw = ws; ws += lay.s2dw_bytes;
  slot[S_STEM] = ws; ws += lay.stem_bytes;
  for (int i = 0; i < 3; ++i) { slot[S_WIDE + i] = ws; ws += lay.wide_bytes; }
  for (int i = 0; i < 2; ++i) { slot[S_NARROW + i] = ws; ws += lay.narrow_bytes; }
  float* stats = reinterpret_cast<float*>(ws); ws += lay.stats_bytes;
  float* fold = reinterpret_cast<float*>(ws);
  const int total = (int)r->bntotal;
  float* fscale = fold; float* fshift = fold + total;

  if (train) {
    if (hipMemsetAsync(stats, 0, lay.stats_bytes, st) != hipSuccess) { st_set_error("memset failed"); return 1; }
  } else {
    hipLaunchKernelGGL(bn_fold_kernel, dim3((total + 255) / 256), dim3(256), 0, st, bn_gamma, bn_beta, bn_running_mean,
                       bn_running_var, fscale, fshift, total, eps);
    ST_LAUNCH_CHECK();
  }
  if (p.s2d) {
    if (st_nchw_to_s2d16(images_nchw, slot[S_IN], dt, B, H, W, stream)) return 1;
  } else if (st_nchw_to_nhwc(images_nchw, slot[S_IN], dt, B, 3, H, W, r->cpad0, stream)) return 1;

  auto S = [&](int s) -> void* { return s == S_NONE ? nullptr : slot[s]; };
  auto wts = [&](size_t off) { return reinterpret_cast<const char*>(weights) + off * es; };
  // the BatchNorm of conv ci as its consumers read it: statistics, gamma, beta, replicas
  struct BnRef { const float* stats; const float* gamma; const float* beta; int rep; };
  auto bn = [&](int ci) { const ConvL& c = r->convs[ci]; return BnRef{stats + tab.soff[ci], bn_gamma + c.bnoff, bn_beta + c.bnoff, tab.rep[ci]}; };
  auto set_in = [&](auto& d, const Launch& l) {    // the producer's BatchNorm + ReLU in the loader
    if (l.in_ci < 0) return;
    const BnRef b = bn(l.in_ci);
    d.in_stats = b.stats; d.in_gamma = b.gamma; d.in_beta = b.beta; d.in_count = tab.count[l.in_ci]; d.in_eps = eps;
  };
  auto set_out = [&](auto& d, const Launch& l) {   // train: replicated statistics; eval: folded BatchNorm (+ReLU) in the epilogue
    const ConvL& c = r->convs[l.ci];
    if (train) { d.stats = stats + tab.soff[l.ci]; d.stats_replicas = l.rep_out; }
    else { d.scale = fscale + c.bnoff; d.shift = fshift + c.bnoff; d.relu = l.relu; }
  };
  auto set_fused = [&](auto& k, const Launch& l) {   // b2b / c3c1: bn2 of the raw input, bn3 of the (re)computed conv3, the identity's BN
    const BnRef b2 = bn(l.in_ci), b3 = bn(l.pc);
    k.bn2_stats = b2.stats; k.bn2_gamma = b2.gamma; k.bn2_beta = b2.beta; k.bn2_replicas = b2.rep;
    k.bn3_stats = b3.stats; k.bn3_gamma = b3.gamma; k.bn3_beta = b3.beta; k.bn3_replicas = b3.rep;
    if (l.id_ci >= 0) { const BnRef i = bn(l.id_ci); k.id_stats = i.stats; k.id_gamma = i.gamma; k.id_beta = i.beta; k.id_replicas = i.rep; }
    k.count = tab.count[l.pc]; k.eps = eps;
  };
  size_t taps_used = 0;
  auto run = [&](const Launch& l) -> int {
    const ConvL& c = r->convs[l.ci];
    const long rows = (long)B * l.hin * l.win;
    switch (l.route) {
      case R_STEM: case R_IGEMM: {
        st_conv_desc d{};
        const int cin_p = c.cin == 3 ? r->cpad0 : c.cin;
        d.x = S(l.x); d.w = wts(c.woff); d.y = S(l.y); d.residual = S(l.res);
        d.dtype = dt; d.out_dtype = dt;
        d.B = B; d.Hin = l.hin; d.Win = l.win; d.Cin = cin_p;
        d.Ho = conv_out(l.hin, c.k, c.stride, c.pad); d.Wo = conv_out(l.win, c.k, c.stride, c.pad);
        d.N = c.cout; d.KH = c.k; d.KW = c.k; d.stride = c.stride; d.pad = c.pad;
        d.ldx = cin_p; d.ldw = c.k * c.k * cin_p; d.ldy = c.cout; d.Cin_logical = c.cin; d.k_order = c.korder;
        if (l.route == R_STEM && p.s2d) {
          if (st_stem_weight_s2d(wts(c.woff), s2dw, dt, r->cpad0, stream)) return 1;
          d.w = s2dw; d.Hin = l.hin / 2 + 3; d.Win = l.win / 2 + 3; d.Cin = 64; d.ldx = 16; d.KH = 4; d.KW = 1; d.stride = 1; d.pad = 0;
          d.ldw = 256; d.Cin_logical = 36;   // 4 rows x 36 = 144 of the 147 real taps: the profiler's FLOP count stays below the algorithmic one
        }
        set_in(d, l); set_out(d, l);
        return st_conv(&d, stream);
      }
      case R_IMG: case R_S2: {
        // image-resident 3x3 (conv_img.hip) / stride-2 K-streaming implicit GEMM with gathered rows (conv_s2.hip)
        st_conv3x3_img_desc g{};
        g.x = S(l.x); g.w_frag = wts(c.woff_frag); g.y = S(l.y);
        g.B = B; g.H = l.hin; g.W = l.win; g.C = c.cin; g.N = c.cout; g.in_stats_replicas = l.rep_in;
        set_in(g, l); set_out(g, l);
        return l.route == R_IMG ? st_conv3x3_img(&g, stream) : st_conv3x3_s2(&g, stream);
      }
      case R_WREG: case R_ASTAT: case R_KSTREAM: {
        st_conv1x1_wreg_desc g{};
        g.x = S(l.x); g.w_frag = wts(c.woff_frag); g.y = S(l.y); g.residual = S(l.res);
        g.B = B; g.Hin = l.hin; g.Win = l.win; g.C = c.cin; g.N = c.cout; g.stride = c.stride; g.in_stats_replicas = l.rep_in;
        set_in(g, l); set_out(g, l);
        if (l.route == R_WREG) return st_conv1x1_wreg(&g, stream);
        if (l.route == R_ASTAT) return st_conv1x1_astat(&g, stream);
        ST_CHECK(!g.in_stats, "st_resnet_forward: the long-K pointwise kernel has no input transform");
        return st_conv1x1_kstream(&g, stream);
      }
      case R_KFUSE: {
        st_conv1x1_kfuse_desc k{};
        const BnRef f = bn(l.pc);
        k.raw = S(l.x); k.identity = S(l.res); k.x_out = S(l.xout); k.w_frag = wts(c.woff_frag); k.y = S(l.y);
        k.stats = stats + tab.soff[l.ci]; k.stats_replicas = l.rep_out;
        k.f_stats = f.stats; k.f_gamma = f.gamma; k.f_beta = f.beta; k.f_count = tab.count[l.pc]; k.f_eps = eps; k.f_stats_replicas = f.rep;
        k.rows = rows; k.C = c.cin; k.N = c.cout;
        if (l.id_ci >= 0) { const BnRef i = bn(l.id_ci); k.id_stats = i.stats; k.id_gamma = i.gamma; k.id_beta = i.beta; k.id_stats_replicas = i.rep; }
        return st_conv1x1_kfuse(&k, stream);
      }
      case R_B2B: case R_B2B0: {
        const ConvL& c3 = r->convs[l.pc];
        st_conv_b2b_desc k{};
        k.raw2 = S(l.x); k.w3_frag = wts(c3.woff_frag); k.identity = S(l.res); k.x_out = S(l.xout);
        set_fused(k, l);
        k.rows = rows; k.C1 = c3.cin; k.C2 = c3.cout;
        if (l.route == R_B2B) {
          k.w1_frag = wts(c.woff_frag); k.y = S(l.y); k.stats = stats + tab.soff[l.ci]; k.stats_replicas = l.rep_out; k.N = c.cout;
        }
        return st_conv_b2b(&k, stream);
      }
      case R_C3C1: {
        const ConvL& c3 = r->convs[l.pc];
        st_conv_c3c1_desc k{};
        k.x2 = S(l.x); k.w3_frag = wts(c3.woff_frag); k.identity = S(l.res); k.x_out = S(l.xout); k.w1_frag = wts(c.woff_frag); k.y = S(l.y);
        if (train) {
          k.stats = stats + tab.soff[l.ci]; k.stats_replicas = l.rep_out;
          set_fused(k, l);
        } else {
          k.scale3 = fscale + c3.bnoff; k.shift3 = fshift + c3.bnoff; k.scale1 = fscale + c.bnoff; k.shift1 = fshift + c.bnoff; k.relu1 = l.relu;
        }
        k.rows = rows; k.C1 = c3.cin; k.C2 = c3.cout; k.N = c.cout;
        return st_conv_c3c1(&k, stream);
      }
      case R_STEM_POOL: {
        // the raw-output buffer is free in this form: 32 KB of it hold the filters
        if (st_stem_weight_frag_packed(wts(c.woff), r->cpad0, slot[S_STEM], stream)) return 1;
        st_stem_conv_pool_desc sd{};
        sd.x_s2d = S(l.x); sd.w_frag = slot[S_STEM]; sd.y = S(l.y); sd.B = B; sd.H = l.hin; sd.W = l.win;
        if (train) { sd.stats = stats + tab.soff[l.ci]; sd.stats_replicas = l.rep_out; sd.gamma = bn_gamma + c.bnoff; }
        else { sd.scale = fscale + c.bnoff; sd.shift = fshift + c.bnoff; }
        return st_stem_conv_pool(&sd, stream);
      }
      case R_MAXPOOL:
        if (l.in_ci < 0) return st_maxpool3x3s2(S(l.x), S(l.y), dt, B, l.hin, l.win, c.cout, stream);
        return st_maxpool3x3s2_bn(S(l.x), S(l.y), dt, B, l.hin, l.win, c.cout, stats + tab.soff[l.ci], bn_gamma + c.bnoff, bn_beta + c.bnoff,
                                  nullptr, nullptr, tab.count[l.ci], eps, stream);
      case R_BN_ACT: {
        st_bn_act_desc d{};
        const BnRef b = bn(l.ci);
        d.x = S(l.x); d.y = S(l.x); d.res = S(l.res);
        d.stats = b.stats; d.stats_replicas = b.rep; d.gamma = b.gamma; d.beta = b.beta;
        if (l.id_ci >= 0) { const BnRef i = bn(l.id_ci); d.res_bn = 1; d.res_stats = i.stats; d.res_stats_replicas = i.rep; d.res_gamma = i.gamma; d.res_beta = i.beta; }
        d.dtype = dt; d.rows = rows; d.C = c.cout; d.count = (float)rows; d.eps = eps; d.relu = 1;
        return st_bn_act(&d, stream);
      }
      case R_REDUCE:
        hipLaunchKernelGGL(bn_reduce_replicas_kernel, dim3((2 * c.cout + 255) / 256), dim3(256), 0, st, stats + tab.soff[l.ci], l.rep_in, 2 * c.cout);
        ST_LAUNCH_CHECK();
        return 0;
      case R_TAP: {      // st_resnet_set_taps: block outputs, one after the other
        if (!r->taps) return 0;
        const size_t nb = (size_t)rows * c.cout * es;
        ST_CHECK(taps_used + nb <= r->taps_bytes, "st_resnet_forward: taps buffer too small (%zu needed so far, %zu given)", taps_used + nb, r->taps_bytes);
        if (hipMemcpyAsync(reinterpret_cast<char*>(r->taps) + taps_used, S(l.x), nb, hipMemcpyDeviceToDevice, st) != hipSuccess) { st_set_error("st_resnet_forward: tap copy failed"); return 1; }
        taps_used += nb;
        return 0;
      }
    }
    return 0;
  };
  FILE* log = layer_log();
  char line[256];
  for (int i = 0; i < p.n; ++i) {
    if (run(p.l[i])) return 1;
    if (log && format_launch(r, B, p.l[i], line, sizeof(line)) > 0) { fputs(line, log); fflush(log); }
  }

  const void* out = slot[p.out];
  const size_t feat_bytes = (size_t)B * p.h * p.w * r->feat_dim * es;
  if (feat_nhwc_out && hipMemcpyAsync(feat_nhwc_out, out, feat_bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) {
    st_set_error("st_resnet_forward: copy failed"); return 1;
  }
  if (pooled_out && st_global_avgpool(out, pooled_out, dt, pooled_dtype, B, p.h * p.w, r->feat_dim, stream)) return 1;
  if (ncp_out && st_nhwc_to_ncp_f32(out, ncp_out, dt, B, p.h * p.w, r->feat_dim, stream)) return 1;

  if (train == 2) {
    std::lock_guard<std::mutex> lk(r->mu);
    r->pending[workspace] = PendingUpdate{tab, stats};
  } else if (train) {
    hipLaunchKernelGGL(bn_update_all_kernel, dim3((total + 255) / 256), dim3(256), 0, st, stats, bn_running_mean,
                       bn_running_var, total, momentum, tab);
    ST_LAUNCH_CHECK();
  }
  return 0;
}


// Second half of a train == 2 forward: the momentum update of every running_mean / running_var from the statistics that
// forward left in `workspace`.  Stream-ordered after that forward by the caller; calls for successive minibatches must be
// ordered among themselves (an event chain when the forwards run on different streams).
extern "C" int st_resnet_update_running(const st_resnet* r, const void* workspace, float* bn_running_mean, float* bn_running_var,
                                        float momentum, void* stream) {
  ST_CHECK(r && workspace && bn_running_mean && bn_running_var, "st_resnet_update_running: null pointer");
  PendingUpdate p;
  {
    std::lock_guard<std::mutex> lk(r->mu);
    auto it = r->pending.find(workspace);
    ST_CHECK(it != r->pending.end(), "st_resnet_update_running: no train == 2 forward is pending for this workspace");
    p = it->second;
    r->pending.erase(it);
  }
  const int total = (int)r->bntotal;
  hipLaunchKernelGGL(bn_update_all_kernel, dim3((total + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p.stats,
                     bn_running_mean, bn_running_var, total, momentum, p.tab);
  ST_LAUNCH_CHECK();
  return 0;
}
