// Host-side plumbing shared by the decoder entry points (rnn.cpp, attn.cpp, decode.hip, sample.hip; decode_pipe.hip and
// head_optim.hip take the rounding and the GEMM helper).  Internal, host-only, not part of the C ABI: ONE definition of the
// workspace rounding, the 1x1-"convolution" GEMM descriptor, the packed-sequence checks and the RnnGemmArgs of a full cell.
#pragma once
#include "common.h"
#include "rnn_kernels.h"
#include <string.h>
#include <vector>

inline size_t st_al256(size_t v) { return (v + 255) & ~(size_t)255; }
inline int st_up8(int v) { return (v + 7) & ~7; }

// Workspace planners carve their buffers in a fixed order, each at a 256-byte boundary; `o` ends as the total.
struct Arena {
  size_t o = 0;
  size_t take(size_t bytes) { const size_t r = o; o += st_al256(bytes); return r; }
};

// y[M][ldy] (out_dtype) (+)= a[M][K] w[N][K]^T (+ bias) as the 1x1 "convolution" st_conv / st_conv_batch run
inline st_conv_desc st_gemm_nt_desc(const void* a, int lda, const void* w, int ldw, void* y, int ldy, int M, int N, int K, int dtype,
                                    int out_dtype, const float* bias, int accumulate = 0, int split_k = 0) {
  st_conv_desc d;
  memset(&d, 0, sizeof(d));
  d.x = a; d.w = w; d.y = y; d.bias = bias; d.dtype = dtype; d.out_dtype = out_dtype;
  d.B = M; d.Hin = 1; d.Win = 1; d.Cin = K; d.Ho = 1; d.Wo = 1; d.N = N; d.KH = 1; d.KW = 1; d.stride = 1; d.pad = 0;
  d.ldx = lda; d.ldw = ldw; d.ldy = ldy; d.accumulate = accumulate; d.split_k = split_k;
  return d;
}
// ... launched on its own.  An empty product is no launch; the decode and head callers never pass 0 rows (they return or fail on
// n <= 0 first), so for them the early return changes nothing.
inline int st_gemm_nt(const void* a, int lda, const void* w, int ldw, void* y, int ldy, int M, int N, int K, int dtype, int out_dtype,
                      const float* bias, void* stream, int accumulate = 0, int split_k = 0) {
  if (M <= 0 || N <= 0) return 0;
  const st_conv_desc d = st_gemm_nt_desc(a, lda, w, ldw, y, ldy, M, N, K, dtype, out_dtype, bias, accumulate, split_k);
  return st_conv(&d, stream);
}

// What both teacher-forced decoders require of a packed sequence: batch sizes positive, non-increasing (captions sorted by
// length, utils.py:66) and adding up to ntok.  The plain decoder gathers its inputs from s->caption itself (need_caption).
inline int st_check_packed_seq(const st_packed_seq* s, const char* who, bool need_caption) {
  ST_CHECK(s->B > 0 && s->T > 0 && s->ntok > 0 && s->batch_sizes_host && s->rows_b && s->rows_t && s->prev_row && (s->caption || !need_caption),
           "%s: bad packed-sequence descriptor", who);
  int sum = 0, prev = s->B;
  for (int t = 0; t < s->T; ++t) {
    const int b = s->batch_sizes_host[t];
    ST_CHECK(b > 0 && b <= prev, "%s: batch_sizes must be positive and non-increasing (captions sorted by length, utils.py:66)", who);
    prev = b; sum += b;
  }
  ST_CHECK(sum == s->ntok && s->batch_sizes_host[0] == s->B, "%s: batch_sizes do not add up to ntok", who);
  return 0;
}

// off[t] = first packed row of step t (row(t, b) = off[t] + b), off[T] = ntok
inline std::vector<int> st_packed_offsets(const st_packed_seq* s) {
  std::vector<int> off(s->T + 1, 0);
  for (int t = 0; t < s->T; ++t) off[t + 1] = off[t] + s->batch_sizes_host[t];
  return off;
}

// A call's dropout (st_dropout, NULL = none) as the entry points use it: which sites are on, their mask keys, and the caller's buffer of
// dropped copies carved into L slots of [ntok][H] rows in the compute dtype (slot l = the dropped output of layer l).
struct DropPlan {
  bool in = false, layer = false, out = false;
  DropKey kin, klayer, kout;
  char* buf = nullptr;
  size_t slot = 0;
  char* rows(int l) const { return buf + (size_t)l * slot; }
  bool any() const { return in || layer || out; }
};
inline size_t st_dropout_buf_bytes(int L, size_t ntok, int H, int dtype) { return (size_t)L * st_al256(ntok * H * st_dtype_size(dtype)); }
// out_only: the attention decoders take p_out alone
inline int st_drop_plan(const st_dropout* d, int L, size_t ntok, int H, int dtype, bool out_only, const char* who, DropPlan* q) {
  *q = DropPlan();
  if (!d) return 0;
  ST_CHECK(d->p_in >= 0.0 && d->p_in < 1.0 && d->p_layer >= 0.0 && d->p_layer < 1.0 && d->p_out >= 0.0 && d->p_out < 1.0,
           "%s: dropout probabilities must be in [0, 1) (p_in=%g, p_layer=%g, p_out=%g)", who, d->p_in, d->p_layer, d->p_out);
  ST_CHECK(d->step >= 0, "%s: dropout step %d is negative", who, d->step);
  ST_CHECK(!out_only || (d->p_in == 0.0 && d->p_layer == 0.0), "%s: this decoder takes p_out only", who);
  q->in = d->p_in > 0.0; q->layer = d->p_layer > 0.0 && L > 1; q->out = d->p_out > 0.0;
  q->kin = drop_key(d->p_in, d->seed, d->step); q->klayer = drop_key(d->p_layer, d->seed, d->step); q->kout = drop_key(d->p_out, d->seed, d->step);
  if (q->layer || q->out) {
    ST_CHECK(d->buf && d->buf_bytes >= st_dropout_buf_bytes(L, ntok, H, dtype), "%s: dropout buffer too small (%zu < %zu)", who,
             d->buf ? d->buf_bytes : (size_t)0, st_dropout_buf_bytes(L, ntok, H, dtype));
    q->buf = reinterpret_cast<char*>(d->buf);
    q->slot = st_al256(ntok * H * st_dtype_size(dtype));
  }
  return 0;
}

// The terms of a loss call (st_loss_terms; the entry points turn NULL into the all-zero descriptor first): smoothing = 1 needs
// label_smoothing in [0, 1) (NaN fails), smoothing = 0 takes none of the smoothing arguments
inline int st_check_loss_terms(const st_loss_terms* t, const char* who) {
  if (t->smoothing) {
    ST_CHECK(t->label_smoothing >= 0.f && t->label_smoothing < 1.f, "%s: label_smoothing=%g outside [0, 1)", who, (double)t->label_smoothing);
  } else {
    ST_CHECK(t->label_smoothing == 0.f && !t->smooth_out && !t->tile_sums,
             "%s: smoothing = 0 takes no label_smoothing, smooth_out or tile_sums (set smoothing = 1 for the label-smoothing kernels)", who);
  }
  return 0;
}

// scheduled sampling (st_rnn_sched_inputs / st_attn_sched_inputs): input_ids = caption, replaced = 0, drawn = -1, logp = 0 before the roll-in
inline int st_sched_init_outputs(const long* caption, int n, int Tcap, long* input_ids, uint8_t* replaced, long* drawn, float* logp, hipStream_t st,
                                 const char* who) {
  const size_t cells = (size_t)n * Tcap;
  if (hipMemcpyAsync(input_ids, caption, cells * sizeof(long), hipMemcpyDeviceToDevice, st) != hipSuccess ||
      hipMemsetAsync(replaced, 0, cells, st) != hipSuccess ||
      (drawn && hipMemsetAsync(drawn, 0xff, cells * sizeof(long), st) != hipSuccess) ||      // every byte 0xff: -1
      (logp && hipMemsetAsync(logp, 0, cells * sizeof(float), st) != hipSuccess)) {
    st_set_error("%s: initialising the outputs failed", who);
    return 1;
  }
  return 0;
}

// Whole-row arg-max (first maximum, like torch.max(1)) of n rows of fp32 logits -> ids[row * ids_stride + t] and, when cur is
// given, cur[row]: csrc/decode.hip, argmax_embed_kernel without its embedding gather.
int argmax_rows_launch(const float* logits, int ldl, int n, int V, long* ids, int ids_stride, int t, long* cur, hipStream_t st);

inline int rnn_cell_epi(int cell) { return cell == ST_CELL_GRU ? 1 : 2; }   // gate epilogue of rnn_gemm_launch*

// RnnGemmArgs of one full (has_x = 1) cell of layer l over M rows: gates from x W_ih^T + b_ih and hprev W_hh^T + b_hh.  x rows are
// `in` wide, every state row H, the optional gate cache (BPTT) 4H.  hprev / cprev NULL = a zero state; cprev / cout are LSTM only.
inline RnnGemmArgs rnn_full_cell(const st_rnn_params* p, int l, const void* x, int in, const void* hprev, const void* cprev,
                                 void* hout, void* cout, int M, void* cache = nullptr) {
  const int H = p->H;
  RnnGemmArgs a;
  memset(&a, 0, sizeof(a));
  a.M = M; a.N = H; a.gstride = H;
  a.A = hprev; a.W = p->w_hh[l]; a.K = H; a.lda = H; a.ldw = H; a.bias_h = p->b_hh[l];
  a.A2 = x; a.W2 = p->w_ih[l]; a.K2 = in; a.lda2 = in; a.ldw2 = in; a.bias_x = p->b_ih[l];
  a.hprev = hprev; a.ldhp = H;
  a.hout = hout; a.ldho = H;
  if (cache) { a.cache = cache; a.ldcache = 4 * H; }
  if (p->cell == ST_CELL_LSTM) { a.cprev = cprev; a.cout = cout; }
  return a;
}
