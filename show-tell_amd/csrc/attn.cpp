// Soft-attention decoder (reference Attention/rnn_attn.py:33-145, rnn_attn_LSTM.py): teacher-forced forward,
// BPTT backward (incl. the doubly-stochastic regulariser of main_attn.py:131) and greedy decoding, each as one
// C-ABI call that issues every kernel of the pass.
//
// Differences from the reference's evaluation ORDER (never from its result):
//   * encoder_att(feat) is time-invariant and computed once per batch (reference: every step, rnn_attn.py:23);
//     its weight gradient is one GEMM over the time-summed d(att1);
//   * hidden state is kept [L][rows][H] (no per-step transposes, rnn_attn.py:70,74); predictions are written
//     straight into time-major packed rows (no (B,T,V) zero tensor + pack, rnn_attn.py:64,72,115).
//
// Backward algebra per step t (rows b < B_t), top layer index L-1, u = att1 + att2:
//   dx0 = [d emb(cap[:,t]) ; d ez]   ez = W_m z + b_m ;  dz = d ez W_m
//   d alpha_p = dz . feat_p + reg_p ; de = alpha (d alpha - <alpha, d alpha>) ; du_p = de_p w_f lrelu'(u_p)
//   d att2 = sum_p du_p ; d att1[b,p] += du_p ; dw_f += sum_p de_p lrelu(u_p) ; db_f += sum_p de_p
//   dh_{t-1}[L-1] += d att2 W_d      (attention at step t is keyed on the PREVIOUS top-layer state)
#include "decoder_host.h"
#include "attn_kernels.h"

namespace {

inline size_t mx(size_t a, size_t b) { return a > b ? a : b; }
// the planners return 0 for a layer count that no entry point accepts
inline bool layers_ok(const st_attn_params* p) { return p->rnn.L >= 1 && p->rnn.L <= ST_MAX_LAYERS; }

// what prepare() fills, at the head of every attention workspace: feat_pf [B*P][F], its mean over P, h0, c0, att1 [B*P][A]
struct AttnPrep {
  size_t feat, mean, h0, c0, att1;
  void take_prep(Arena& ar, const st_attn_params* p, size_t B) {
    const size_t es = st_dtype_size(p->rnn.dtype), H = p->rnn.H;
    feat = ar.take(B * p->P * p->F * es);
    mean = ar.take(B * p->F * es);
    h0 = ar.take(B * H * es);
    c0 = ar.take(B * H * es);
    att1 = ar.take(B * p->P * p->A * es);
  }
};

struct Plan : AttnPrep {
  int G, GH, Np, Vp, BP;
  size_t es;
  size_t xp, y, gates, cst, z, att2, tokT;
  size_t dytop, dxa, dxb, dhc, dcc, dgx, dgh, dez, datt2p, datt2, dz, datt1, dalpha, hprev, tA, tB, wThh, wTih, wTmisc, cast, total;
};

Plan make_plan(const st_attn_params* p, const st_packed_seq* s) {
  const st_rnn_params& r = p->rnn;
  Plan q;
  q.G = r.cell == ST_CELL_GRU ? 3 : 4;
  q.GH = q.G * r.H;
  q.BP = s->B * p->P;
  q.Np = st_up8(s->ntok > q.BP ? s->ntok : q.BP);
  q.Vp = st_up8(r.V);
  q.es = st_dtype_size(r.dtype);
  const size_t n = s->ntok, L = r.L, H = r.H, E = r.E, B = s->B, es = q.es;
  Arena ar;
  q.take_prep(ar, p, B);
  q.xp = ar.take(n * 2 * E * es);
  q.y = ar.take(L * n * H * es);
  q.gates = ar.take(L * n * 4 * H * es);
  q.cst = ar.take(r.cell == ST_CELL_LSTM ? L * n * H * es : 0);
  q.z = ar.take(n * p->F * es);
  q.att2 = ar.take(n * p->A * sizeof(float));
  q.tokT = 0;
  // backward
  q.dytop = ar.take(n * H * sizeof(float));
  const size_t wmax = mx(H, 2 * E);
  q.dxa = ar.take(B * wmax * sizeof(float));
  q.dxb = ar.take(B * wmax * sizeof(float));
  q.dhc = ar.take(L * B * H * sizeof(float));
  q.dcc = ar.take(L * B * H * sizeof(float));
  q.dgx = ar.take(L * n * q.GH * es);
  q.dgh = ar.take(r.cell == ST_CELL_GRU ? L * n * q.GH * es : 0);
  q.dez = ar.take(n * E * es);
  q.datt2p = ar.take(n * p->A * es);
  q.datt2 = ar.take(B * p->A * sizeof(float));
  q.dz = ar.take(B * p->F * sizeof(float));
  q.datt1 = ar.take((size_t)q.BP * p->A * sizeof(float));
  q.dalpha = ar.take((size_t)q.BP * sizeof(float));
  q.hprev = ar.take(n * H * es);
  const size_t ra = mx(mx((size_t)r.V, (size_t)q.GH), mx((size_t)p->A, mx(E, H)));
  const size_t rb = mx(mx((size_t)p->F, 2 * E), H);
  q.tA = ar.take(ra * q.Np * es);
  q.tB = ar.take(rb * q.Np * es);
  q.wThh = ar.take(L * H * q.GH * es);
  q.wTih = ar.take(L * wmax * q.GH * es);
  q.wTmisc = ar.take(mx(mx((size_t)H * q.Vp, (size_t)p->F * E), (size_t)H * p->A) * es);
  q.cast = ar.take(mx(mx((size_t)q.BP * p->A, B * H), (size_t)H * p->A) * es);
  q.total = ar.o;
  return q;
}

// A[M][K] W[N][K]^T (+bias) through the skinny MFMA kernel, for the <= batch rows of one timestep: out is fp32 [M][ldo], (+)=; or,
// with to_storage, storage-dtype rows (the per-step context embedding, [B_t x F] x [F x E] with K = 2048: 4 output tiles of a
// 128x128 MFMA tile walk K for ~37 us, 128 blocks of 16x16 with K split over 4 waves for ~10)
int skinny(const void* A, int lda, const void* W, int ldw, void* out, int ldo, int M, int N, int K, const float* bias, int accumulate,
           int dtype, hipStream_t st, bool to_storage = false) {
  RnnGemmArgs a;
  memset(&a, 0, sizeof(a));
  a.A = A; a.W = W; a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldw = ldw; a.gstride = 0; a.bias_h = bias;
  if (to_storage) { a.hout = out; a.ldho = ldo; }
  else { a.out_f32 = reinterpret_cast<float*>(out); a.ldo = ldo; a.accumulate = accumulate; }
  return rnn_gemm_launch(a, dtype, 0, 0, st);
}

int check_common(const st_attn_params* p, const st_packed_seq* s, const char* who) {
  ST_CHECK(p, "%s: null descriptor", who);
  const st_rnn_params& r = p->rnn;
  ST_CHECK(r.cell == ST_CELL_GRU || r.cell == ST_CELL_LSTM, "%s: bad cell", who);
  ST_CHECK(r.L >= 1 && r.L <= ST_MAX_LAYERS, "%s: bad layer count %d", who, r.L);
  ST_CHECK(r.in0 == 2 * r.E, "%s: the attention decoder's layer-0 input is 2*embed_dim (rnn_attn.py:50)", who);
  ST_CHECK(r.H % 8 == 0 && r.E % 8 == 0 && p->A % 8 == 0 && p->F % 8 == 0, "%s: need H, E, A and F multiples of 8 (H=%d E=%d A=%d F=%d)",
           who, r.H, r.E, p->A, p->F);
  ST_CHECK(p->P >= 1 && p->P <= 64, "%s: at most 64 pixels (P=%d)", who, p->P);
  ST_CHECK(p->w_enc && p->b_enc && p->w_dec && p->b_dec && p->w_full && p->b_full && p->w_init_h && p->b_init_h && p->w_embed && p->b_embed && r.emb,
           "%s: null attention weights", who);
  ST_CHECK(r.cell == ST_CELL_GRU || (p->w_init_c && p->b_init_c), "%s: LSTM needs init_c", who);
  if (s) {
    if (st_check_packed_seq(s, who, false)) return 1;        // the captions come as caption_T, not through s->caption
    ST_CHECK(s->Tcap >= s->T, "%s: caption width %d smaller than the longest length %d", who, s->Tcap, s->T);
  }
  return 0;
}

// feat_pf, mean, h0 (c0), att1 -- shared by training and the searches
int prepare(const st_attn_params* p, const float* cnn_feature, int B, char* ws, const AttnPrep& q, void* stream) {
  char *feat = ws + q.feat, *mean = ws + q.mean, *h0 = ws + q.h0, *c0 = ws + q.c0, *att1 = ws + q.att1;
  const st_rnn_params& r = p->rnn;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int dt = r.dtype, BP = B * p->P;
  if (ncp_to_pf_launch(cnn_feature, feat, B, p->F, p->P, dt, st)) return 1;
  if (st_global_avgpool(feat, mean, dt, dt, B, p->P, p->F, stream)) return 1;                        // cnn_feature.mean(dim=2), rnn_attn.py:62
  if (st_gemm_nt(mean, p->F, p->w_init_h, p->F, h0, r.H, B, r.H, p->F, dt, dt, p->b_init_h, stream)) return 1;
  if (r.cell == ST_CELL_LSTM && st_gemm_nt(mean, p->F, p->w_init_c, p->F, c0, r.H, B, r.H, p->F, dt, dt, p->b_init_c, stream)) return 1;
  return st_gemm_nt(feat, p->F, p->w_enc, p->F, att1, p->A, BP, p->A, p->F, dt, dt, p->b_enc, stream);   // hoisted encoder_att
}

}  // namespace

extern "C" size_t st_attn_workspace_bytes(const st_attn_params* p, const st_packed_seq* s) {
  if (!p || !s || !layers_ok(p)) return 0;
  return make_plan(p, s).total;
}

// Dropout (st_dropout, NULL = none): the Show-Attend-Tell placement, in front of `linear` only.  The recurrence and the next step's
// attention read the plain top state; the dropped copy of y_top (the caller's buffer) feeds the projection and dW_lin, and dy_top is
// masked before the step loop of the backward pass.
extern "C" int st_attn_forward(const st_attn_params* p, const st_packed_seq* s, const float* cnn_feature, const long* caption_T,
                               void* workspace, size_t workspace_bytes, void* logits, int logits_dtype, int ldl,
                               float* alphas, int save_for_backward, const st_dropout* drop, void* stream) {
  if (check_common(p, s, "st_attn_forward")) return 1;
  DropPlan dp;
  if (st_drop_plan(drop, p->rnn.L, s->ntok, p->rnn.H, p->rnn.dtype, true, "st_attn_forward", &dp)) return 1;
  ST_CHECK(cnn_feature && caption_T && workspace && alphas, "st_attn_forward: null pointer");
  const Plan q = make_plan(p, s);
  ST_CHECK(workspace_bytes >= q.total, "st_attn_forward: workspace too small (%zu < %zu)", workspace_bytes, q.total);
  const st_rnn_params& r = p->rnn;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* ws = reinterpret_cast<char*>(workspace);
  const int dt = r.dtype, H = r.H, E = r.E, n = s->ntok, B = s->B, L = r.L, P = p->P, A = p->A, F = p->F;
  const size_t es = q.es;
  (void)save_for_backward;   // every saved tensor is also the forward's own scratch
  const std::vector<int> off = st_packed_offsets(s);

  if (prepare(p, cnn_feature, B, ws, q, stream)) return 1;

  for (int t = 0; t < s->T; ++t) {
    const int bt = s->batch_sizes_host[t];
    const char* htop_prev = t > 0 ? ws + q.y + ((size_t)(L - 1) * n + off[t - 1]) * H * es : ws + q.h0;
    float* att2 = reinterpret_cast<float*>(ws + q.att2) + (size_t)off[t] * A;
    char* zt = ws + q.z + (size_t)off[t] * F * es;
    char* xt = ws + q.xp + (size_t)off[t] * 2 * E * es;
    if (skinny(htop_prev, H, p->w_dec, H, att2, A, bt, A, H, p->b_dec, 0, dt, st)) return 1;
    if (attn_fwd_launch(ws + q.att1, att2, p->w_full, p->b_full, ws + q.feat, alphas + (size_t)t * P, (long)s->Tcap * P, zt, bt, P, A, F, dt, st)) return 1;
    if (st_embedding_rows(r.emb, caption_T + (size_t)t * B, xt, bt, E, r.V, 2 * E, dt, stream)) return 1;
    if (skinny(zt, F, p->w_embed, F, xt + (size_t)E * es, 2 * E, bt, E, F, p->b_embed, 0, dt, st, true)) return 1;
    for (int l = 0; l < L; ++l) {
      char* yl = ws + q.y + (size_t)l * n * H * es;
      char* cl = ws + q.cst + (size_t)l * n * H * es;
      // every layer starts from the same h0 (c0) (rnn_attn.py:62)
      const RnnGemmArgs a = rnn_full_cell(&r, l, l == 0 ? xt : ws + q.y + ((size_t)(l - 1) * n + off[t]) * H * es, l == 0 ? 2 * E : H,
                                          t > 0 ? yl + (size_t)off[t - 1] * H * es : ws + q.h0, t > 0 ? cl + (size_t)off[t - 1] * H * es : ws + q.c0,
                                          yl + (size_t)off[t] * H * es, cl + (size_t)off[t] * H * es, bt,
                                          ws + q.gates + ((size_t)l * n + off[t]) * 4 * H * es);
      if (rnn_gemm_launch(a, dt, rnn_cell_epi(r.cell), 1, st)) return 1;
    }
  }
  const char* ytop = ws + q.y + (size_t)(L - 1) * n * H * es;
  if (dp.out) {
    if (dropout_rows_launch(ytop, dp.rows(L - 1), dt, n, H, H, H, dp.kout, L - 1, 0, st)) return 1;
    ytop = dp.rows(L - 1);
  }
  if (logits) {
    ST_CHECK(r.w_lin && r.b_lin, "st_attn_forward: logits requested without the vocabulary projection");
    if (st_gemm_nt(ytop, H, r.w_lin, H, logits, ldl, n, r.V, H, dt, logits_dtype, r.b_lin, stream)) return 1;
  }
  return 0;
}
extern "C" size_t st_attn_dropout_bytes(const st_attn_params* p, const st_packed_seq* s) {
  if (!p || !s) return 0;
  return st_dropout_buf_bytes(p->rnn.L, s->ntok, p->rnn.H, p->rnn.dtype);
}

extern "C" int st_attn_reg_loss(const float* alphas, int B, int T, int P, float alpha_c, float* loss_accum, void* stream) {
  ST_CHECK(alphas && loss_accum, "st_attn_reg_loss: null pointer");
  return attn_reg_launch(alphas, B, T, P, alpha_c, loss_accum, nullptr, nullptr, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int st_attn_backward(const st_attn_params* p, const st_attn_grads* g, const st_packed_seq* s, const long* caption_T,
                                const void* dlogits, int ldd, const float* alphas, const float* dalphas, float alpha_c,
                                const float* grad_scale_dev, void* workspace, size_t workspace_bytes, const st_dropout* drop, void* stream) {
  if (check_common(p, s, "st_attn_backward")) return 1;
  DropPlan dp;
  if (st_drop_plan(drop, p->rnn.L, s->ntok, p->rnn.H, p->rnn.dtype, true, "st_attn_backward", &dp)) return 1;
  ST_CHECK(g && caption_T && dlogits && alphas && workspace, "st_attn_backward: null pointer");
  const Plan q = make_plan(p, s);
  ST_CHECK(workspace_bytes >= q.total, "st_attn_backward: workspace too small (%zu < %zu)", workspace_bytes, q.total);
  const st_rnn_params& r = p->rnn;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* ws = reinterpret_cast<char*>(workspace);
  const int dt = r.dtype, H = r.H, E = r.E, n = s->ntok, B = s->B, L = r.L, P = p->P, A = p->A, F = p->F, GH = q.GH, Np = q.Np, BP = q.BP;
  const size_t es = q.es;
  ST_CHECK(ldd >= q.Vp && ldd % 8 == 0, "st_attn_backward: dlogits leading dimension must be a multiple of 8 and >= %d", q.Vp);
  ST_CHECK(Np >= n && Np >= BP, "st_attn_backward: plan Np=%d n=%d BP=%d P=%d B=%d T=%d", Np, n, BP, P, B, s->T);
  const std::vector<int> off = st_packed_offsets(s);
  const char* ytop = dp.out ? dp.rows(L - 1) : ws + q.y + (size_t)(L - 1) * n * H * es;   // what `linear` read
  float* dytop = reinterpret_cast<float*>(ws + q.dytop);
  float* dhc = reinterpret_cast<float*>(ws + q.dhc);
  float* dcc = reinterpret_cast<float*>(ws + q.dcc);
  float* datt1 = reinterpret_cast<float*>(ws + q.datt1);
  float* dalpha = reinterpret_cast<float*>(ws + q.dalpha);
  float* dz = reinterpret_cast<float*>(ws + q.dz);
  float* datt2 = reinterpret_cast<float*>(ws + q.datt2);

  // vocabulary projection
  if (st_transpose_colsum(dlogits, ws + q.tA, g->rnn.b_lin, dt, n, r.V, ldd, Np, stream)) return 1;
  if (st_transpose(ytop, ws + q.tB, dt, n, H, H, Np, stream)) return 1;
  if (st_gemm_nt(ws + q.tA, Np, ws + q.tB, Np, g->rnn.w_lin, H, r.V, H, Np, dt, ST_F32, nullptr, stream, 1)) return 1;
  if (st_transpose(r.w_lin, ws + q.wTmisc, dt, r.V, H, H, q.Vp, stream)) return 1;
  if (st_gemm_nt(dlogits, ldd, ws + q.wTmisc, q.Vp, dytop, H, n, H, q.Vp, dt, ST_F32, nullptr, stream)) return 1;
  if (dp.out && dropout_rows_launch(dytop, dytop, ST_F32, n, H, H, H, dp.kout, L - 1, 0, st)) return 1;   // d dropped y_top -> d y_top

  // transposed operands used inside the time loop
  for (int l = 0; l < L; ++l) {
    const int in = l == 0 ? 2 * E : H;
    if (st_transpose(r.w_hh[l], ws + q.wThh + (size_t)l * H * GH * es, dt, GH, H, H, GH, stream)) return 1;
    if (st_transpose(r.w_ih[l], ws + q.wTih + (size_t)l * mx(H, 2 * E) * GH * es, dt, GH, in, in, GH, stream)) return 1;
  }
  char* wTembed = ws + q.wTmisc;                                   // [F][E]   (w_lin^T is no longer needed)
  if (st_transpose(p->w_embed, wTembed, dt, E, F, F, E, stream)) return 1;
  char* wTdec = ws + q.cast;                                       // [H][A]
  if (st_transpose(p->w_dec, wTdec, dt, A, H, H, A, stream)) return 1;

  if (hipMemsetAsync(dhc, 0, (size_t)L * B * H * sizeof(float), st) != hipSuccess ||
      hipMemsetAsync(dcc, 0, (size_t)L * B * H * sizeof(float), st) != hipSuccess ||
      hipMemsetAsync(datt1, 0, (size_t)BP * A * sizeof(float), st) != hipSuccess) { st_set_error("memset failed"); return 1; }
  if (!dalphas && attn_reg_launch(alphas, B, s->Tcap, P, alpha_c, nullptr, dalpha, grad_scale_dev, st)) return 1;

  for (int t = s->T - 1; t >= 0; --t) {
    const int bt = s->batch_sizes_host[t];
    const float* dy = dytop + (size_t)off[t] * H;
    float* dxa = reinterpret_cast<float*>(ws + q.dxa);
    float* dxb = reinterpret_cast<float*>(ws + q.dxb);
    for (int l = L - 1; l >= 0; --l) {
      const int in = l == 0 ? 2 * E : H;
      char* yl = ws + q.y + (size_t)l * n * H * es;
      const void* hprev = t > 0 ? yl + (size_t)off[t - 1] * H * es : ws + q.h0;
      char* dgx = ws + q.dgx + ((size_t)l * n + off[t]) * GH * es;
      char* dgh = r.cell == ST_CELL_GRU ? ws + q.dgh + ((size_t)l * n + off[t]) * GH * es : dgx;
      const char* cache = ws + q.gates + ((size_t)l * n + off[t]) * 4 * H * es;
      float* dhl = dhc + (size_t)l * B * H;
      if (r.cell == ST_CELL_GRU) {
        if (gru_bwd_gates_launch(dy, dhl, cache, hprev, dgx, dgh, bt, H, dt, st)) return 1;
      } else {
        char* cl = ws + q.cst + (size_t)l * n * H * es;
        const void* cprev = t > 0 ? cl + (size_t)off[t - 1] * H * es : ws + q.c0;
        if (lstm_bwd_gates_launch(dy, dhl, dcc + (size_t)l * B * H, cache, cl + (size_t)off[t] * H * es, cprev, dgx, bt, H, dt, st)) return 1;
      }
      // dh_{t-1}[l] += dgh W_hh   (also at t == 0: the gradient reaches h0 -> init_h)
      if (skinny(dgh, GH, ws + q.wThh + (size_t)l * H * GH * es, GH, dhl, H, bt, H, GH, nullptr, 1, dt, st)) return 1;
      // dx_l = dgx W_ih
      if (skinny(dgx, GH, ws + q.wTih + (size_t)l * mx(H, 2 * E) * GH * es, GH, dxa, in, bt, in, GH, nullptr, 0, dt, st)) return 1;
      dy = dxa;
      float* tmp = dxa; dxa = dxb; dxb = tmp;
    }
    // dy now holds dx0 [bt][2E]
    char* dez = ws + q.dez + (size_t)off[t] * E * es;
    if (split_dx0_launch(dy, caption_T + (size_t)t * B, g->rnn.emb, dez, bt, E, r.V, dt, st)) return 1;
    if (skinny(dez, E, wTembed, E, dz, F, bt, F, E, nullptr, 0, dt, st)) return 1;                  // dz = d ez W_embed
    const float* att2 = reinterpret_cast<const float*>(ws + q.att2) + (size_t)off[t] * A;
    if (attn_bwd_launch(dz, dalphas ? dalphas + (size_t)t * P : dalpha, dalphas ? (long)s->Tcap * P : (long)P, alphas + (size_t)t * P, (long)s->Tcap * P,
                        ws + q.att1, att2, p->w_full, ws + q.feat,
                        datt2, datt1, g->w_full, g->b_full, bt, P, A, F, dt, st)) return 1;
    char* datt2p = ws + q.datt2p + (size_t)off[t] * A * es;
    if (st_cast(datt2, datt2p, ST_F32, dt, (long)bt * A, stream)) return 1;
    // the attention of step t was keyed on the top layer's PREVIOUS state
    if (skinny(datt2p, A, wTdec, A, dhc + (size_t)(L - 1) * B * H, H, bt, H, A, nullptr, 1, dt, st)) return 1;
  }

  // ---- parameter gradients as large GEMMs over the packed rows -------------------------------------------
  for (int l = 0; l < L; ++l) {
    const int in = l == 0 ? 2 * E : H;
    const char* xl = l == 0 ? ws + q.xp : ws + q.y + (size_t)(l - 1) * n * H * es;
    char* dgx = ws + q.dgx + (size_t)l * n * GH * es;
    char* dgh = r.cell == ST_CELL_GRU ? ws + q.dgh + (size_t)l * n * GH * es : dgx;
    if (r.cell != ST_CELL_GRU && colsum_launch(dgh, g->rnn.b_hh[l], n, GH, GH, dt, st)) return 1;   // LSTM: dgh == dgx
    if (st_transpose_colsum(dgx, ws + q.tA, g->rnn.b_ih[l], dt, n, GH, GH, Np, stream)) return 1;
    if (st_transpose(xl, ws + q.tB, dt, n, in, in, Np, stream)) return 1;
    if (st_gemm_nt(ws + q.tA, Np, ws + q.tB, Np, g->rnn.w_ih[l], in, GH, in, Np, dt, ST_F32, nullptr, stream, 1)) return 1;
    if (gather_hprev_launch(ws + q.y + (size_t)l * n * H * es, s->rows_t, s->prev_row, ws + q.hprev, n, H, dt, st, ws + q.h0, s->rows_b)) return 1;
    if (r.cell == ST_CELL_GRU && st_transpose_colsum(dgh, ws + q.tA, g->rnn.b_hh[l], dt, n, GH, GH, Np, stream)) return 1;
    if (st_transpose(ws + q.hprev, ws + q.tB, dt, n, H, H, Np, stream)) return 1;
    if (st_gemm_nt(ws + q.tA, Np, ws + q.tB, Np, g->rnn.w_hh[l], H, GH, H, Np, dt, ST_F32, nullptr, stream, 1)) return 1;
  }
  // decoder_att: d att2 rows x previous top state (hprev of the last layer is still in q.hprev / tB)
  if (st_transpose_colsum(ws + q.datt2p, ws + q.tA, g->b_dec, dt, n, A, A, Np, stream)) return 1;
  if (st_gemm_nt(ws + q.tA, Np, ws + q.tB, Np, g->w_dec, H, A, H, Np, dt, ST_F32, nullptr, stream, 1)) return 1;
  // embed: d ez rows x z rows
  if (st_transpose_colsum(ws + q.dez, ws + q.tA, g->b_embed, dt, n, E, E, Np, stream)) return 1;
  if (st_transpose(ws + q.z, ws + q.tB, dt, n, F, F, Np, stream)) return 1;
  if (st_gemm_nt(ws + q.tA, Np, ws + q.tB, Np, g->w_embed, F, E, F, Np, dt, ST_F32, nullptr, stream, 1)) return 1;
  // encoder_att: time-summed d att1 (B*P rows) x feat
  if (st_cast(datt1, ws + q.cast, ST_F32, dt, (long)BP * A, stream)) return 1;
  if (st_transpose_colsum(ws + q.cast, ws + q.tA, g->b_enc, dt, BP, A, A, Np, stream)) return 1;
  if (st_transpose(ws + q.feat, ws + q.tB, dt, BP, F, F, Np, stream)) return 1;
  if (st_gemm_nt(ws + q.tA, Np, ws + q.tB, Np, g->w_enc, F, A, F, Np, dt, ST_F32, nullptr, stream, 1)) return 1;
  // init_h (init_c): every layer started from the same h0, so its gradient is the sum over layers
  const int Bp = st_up8(B);
  for (int pass = 0; pass < (r.cell == ST_CELL_LSTM ? 2 : 1); ++pass) {
    float* acc = pass == 0 ? dhc : dcc;
    for (int l = 1; l < L; ++l) if (add_rows_launch(acc, acc + (size_t)l * B * H, (long)B * H, st)) return 1;
    if (st_cast(acc, ws + q.cast, ST_F32, dt, (long)B * H, stream)) return 1;
    float* gw = pass == 0 ? g->w_init_h : g->w_init_c;
    float* gb = pass == 0 ? g->b_init_h : g->b_init_c;
    if (st_transpose_colsum(ws + q.cast, ws + q.tA, gb, dt, B, H, H, Bp, stream)) return 1;
    if (st_transpose(ws + q.mean, ws + q.tB, dt, B, F, F, Bp, stream)) return 1;
    if (st_gemm_nt(ws + q.tA, Bp, ws + q.tB, Bp, gw, F, H, F, Bp, dt, ST_F32, nullptr, stream, 1)) return 1;
  }
  return 0;
}

// ---- greedy decoding (rnn_attn.py:77-94,120-145) -----------------------------------------------------------
namespace {
struct GPlan : AttnPrep { size_t h[2], c[2], x, z, att2, logits, ids, total; };
GPlan make_gplan(const st_attn_params* p, int B) {
  const st_rnn_params& r = p->rnn;
  const size_t es = st_dtype_size(r.dtype);
  GPlan q; Arena ar;
  q.take_prep(ar, p, B);
  for (int i = 0; i < 2; ++i) { q.h[i] = ar.take((size_t)r.L * B * r.H * es); q.c[i] = ar.take((size_t)r.L * B * r.H * es); }
  q.x = ar.take((size_t)B * 2 * r.E * es); q.z = ar.take((size_t)B * p->F * es);
  q.att2 = ar.take((size_t)B * p->A * sizeof(float));
  q.logits = ar.take((size_t)B * st_up8(r.V) * sizeof(float));
  q.ids = ar.take((size_t)B * sizeof(long) + (size_t)B * p->P * sizeof(float));
  q.total = ar.o;
  return q;
}

__global__ void fill_ids_kernel(long* cur, int n, long v) { const int i = blockIdx.x * blockDim.x + threadIdx.x; if (i < n) cur[i] = v; }
}  // namespace

extern "C" size_t st_attn_greedy_workspace_bytes(const st_attn_params* p, int B) {
  if (!p || B <= 0 || !layers_ok(p)) return 0;
  return make_gplan(p, B).total;
}

namespace {
// how a step turns its logits into the next token: NULL = arg-max (rnn_attn.py:141), else a draw by st_sample_rows
struct SampleSpec { const float* u; float inv_temperature; int top_k; float top_p; long end_id; float* logp_out; };
// scheduled sampling's roll-in (st_attn_sched_inputs): step 0 reads the captions' first column, step t's logits decide slot t + 1 by
// st_sample_mix_rows, which also hands the next step its token
struct MixSpec { const long* caption_T; int Tcap; const int* lens; const float* coin; const float* u; float prob, inv_temperature; int top_k;
                 long* input_ids; uint8_t* replaced; long* drawn; float* logp; };

// rnn_attn.py:120-145; alphas_out [B][steps][P] keeps every step's attention map (else it goes to a scratch row).
// The greedy and the sampling searches share this loop; sampling keeps its per-row finished bytes behind the greedy plan.
int attn_greedy_run(const st_attn_params* p, const float* cnn_feature, int B, int steps, long start_id, void* workspace,
                    size_t workspace_bytes, long* ids_out, float* alphas_out, void* stream, const char* who, const SampleSpec* sp = nullptr,
                    const MixSpec* mix = nullptr) {
  if (check_common(p, nullptr, who)) return 1;
  ST_CHECK(cnn_feature && workspace && (ids_out || mix) && B > 0 && steps > 0, "%s: bad arguments", who);
  const st_rnn_params& r = p->rnn;
  ST_CHECK(r.w_lin && r.b_lin, "%s: null vocabulary projection", who);
  const GPlan q = make_gplan(p, B);
  ST_CHECK(workspace_bytes >= q.total + (sp ? st_al256((size_t)B) : 0), "%s: workspace too small", who);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* ws = reinterpret_cast<char*>(workspace);
  uint8_t* fin = reinterpret_cast<uint8_t*>(ws + q.total);
  if (sp && hipMemsetAsync(fin, 0, (size_t)B, st) != hipSuccess) { st_set_error("%s: memset failed", who); return 1; }
  const int dt = r.dtype, H = r.H, E = r.E, L = r.L, P = p->P, A = p->A, F = p->F, Vp = st_up8(r.V);
  const size_t es = st_dtype_size(dt);
  if (prepare(p, cnn_feature, B, ws, q, stream)) return 1;
  if (replicate_rows_launch(ws + q.h0, ws + q.h[0], (long)B * H, L, dt, st)) return 1;            // h0 repeated over layers (rnn_attn.py:62)
  if (r.cell == ST_CELL_LSTM && replicate_rows_launch(ws + q.c0, ws + q.c[0], (long)B * H, L, dt, st)) return 1;
  long* cur = reinterpret_cast<long*>(ws + q.ids);
  float* alpha_scratch = reinterpret_cast<float*>(ws + q.ids + (size_t)B * sizeof(long));
  if (!mix) {
    hipLaunchKernelGGL(fill_ids_kernel, dim3((B + 255) / 256), dim3(256), 0, st, cur, B, start_id);
    ST_LAUNCH_CHECK();
  }
  float* att2 = reinterpret_cast<float*>(ws + q.att2);
  float* logits = reinterpret_cast<float*>(ws + q.logits);
  int c = 0;
  for (int t = 0; t < steps; ++t) {
    const int nx = c ^ 1;
    const char* htop = ws + q.h[c] + (size_t)(L - 1) * B * H * es;
    float* alpha_t = alphas_out ? alphas_out + (size_t)t * P : alpha_scratch;
    const long alpha_stride = alphas_out ? (long)steps * P : (long)P;
    if (skinny(htop, H, p->w_dec, H, att2, A, B, A, H, p->b_dec, 0, dt, st)) return 1;
    if (attn_fwd_launch(ws + q.att1, att2, p->w_full, p->b_full, ws + q.feat, alpha_t, alpha_stride, ws + q.z, B, P, A, F, dt, st)) return 1;
    if (st_embedding_rows(r.emb, mix && t == 0 ? mix->caption_T : cur, ws + q.x, B, E, r.V, 2 * E, dt, stream)) return 1;
    if (skinny(ws + q.z, F, p->w_embed, F, ws + q.x + (size_t)E * es, 2 * E, B, E, F, p->b_embed, 0, dt, st, true)) return 1;
    if (st_rnn_step(&r, ws + q.x, B, ws + q.h[c], ws + q.c[c], ws + q.h[nx], ws + q.c[nx], logits, Vp, stream)) return 1;
    if (mix) {                                     // slot t + 1 of caption_T [Tcap][B]: row stride 1, column offset (t + 1) * B
      if (st_sample_mix_rows(logits, Vp, B, r.V, mix->u + t + 1, mix->Tcap, mix->inv_temperature, mix->top_k, mix->coin + t + 1, mix->Tcap, mix->prob,
                             mix->caption_T, 1, (long)(t + 1) * B, mix->lens, t + 1, mix->drawn, mix->logp, mix->input_ids, mix->replaced, mix->Tcap,
                             t + 1, cur, stream)) return 1;
    } else if (sp) {
      if (st_sample_rows_topp(logits, Vp, B, r.V, sp->u + t, steps, sp->inv_temperature, sp->top_k, sp->top_p, sp->end_id, fin, ids_out, sp->logp_out,
                              steps, t, cur, stream)) return 1;
    } else if (argmax_rows_launch(logits, Vp, B, r.V, ids_out, steps, t, cur, st)) return 1;   // first maximum, like torch.max (rnn_attn.py:141)
    c = nx;
  }
  return 0;
}
}  // namespace

extern "C" int st_attn_greedy(const st_attn_params* p, const float* cnn_feature, int B, int steps, long start_id,
                              void* workspace, size_t workspace_bytes, long* ids_out, void* stream) {
  return attn_greedy_run(p, cnn_feature, B, steps, start_id, workspace, workspace_bytes, ids_out, nullptr, stream, "st_attn_greedy");
}

extern "C" int st_attn_greedy_alphas(const st_attn_params* p, const float* cnn_feature, int B, int steps, long start_id,
                                     void* workspace, size_t workspace_bytes, long* ids_out, float* alphas_out, void* stream) {
  ST_CHECK(alphas_out, "st_attn_greedy_alphas: null alphas_out");
  return attn_greedy_run(p, cnn_feature, B, steps, start_id, workspace, workspace_bytes, ids_out, alphas_out, stream, "st_attn_greedy_alphas");
}

extern "C" size_t st_attn_sample_workspace_bytes(const st_attn_params* p, int n) {
  if (!p || n <= 0 || !layers_ok(p)) return 0;
  return make_gplan(p, n).total + st_al256((size_t)n);
}

extern "C" int st_attn_sample(const st_attn_params* p, const float* cnn_feature, int n, int steps, long start_id, const float* u,
                              float inv_temperature, int top_k, long end_id, void* workspace, size_t workspace_bytes,
                              long* ids_out, float* logp_out, float* alphas_out, void* stream) {
  return st_attn_sample_topp(p, cnn_feature, n, steps, start_id, u, inv_temperature, top_k, 1.f, end_id, workspace, workspace_bytes, ids_out, logp_out,
                             alphas_out, stream);
}

extern "C" int st_attn_sample_topp(const st_attn_params* p, const float* cnn_feature, int n, int steps, long start_id, const float* u,
                                   float inv_temperature, int top_k, float top_p, long end_id, void* workspace, size_t workspace_bytes,
                                   long* ids_out, float* logp_out, float* alphas_out, void* stream) {
  ST_CHECK(top_p > 0.f && top_p <= 1.f, "st_attn_sample: need 0 < top_p <= 1 (got %g)", (double)top_p);
  ST_CHECK(u && logp_out, "st_attn_sample: null pointer");
  const SampleSpec sp = {u, inv_temperature, top_k, top_p, end_id, logp_out};
  return attn_greedy_run(p, cnn_feature, n, steps, start_id, workspace, workspace_bytes, ids_out, alphas_out, stream, "st_attn_sample", &sp);
}

// ---- scheduled sampling: the roll-in of the attention decoders (the loop above following the caption) -----------------------------
extern "C" size_t st_attn_sched_inputs_workspace_bytes(const st_attn_params* p, int n) {
  if (!p || n <= 0 || !layers_ok(p)) return 0;
  return make_gplan(p, n).total;
}

extern "C" int st_attn_sched_inputs(const st_attn_params* p, const float* cnn_feature, int n, const long* caption, const long* caption_T, int Tcap,
                                    const int* lens, int max_len, const float* coin, const float* u, float prob, float inv_temperature, int top_k,
                                    void* workspace, size_t workspace_bytes, long* input_ids, uint8_t* replaced, long* drawn, float* logp,
                                    void* stream) {
  ST_CHECK(caption && caption_T && lens && coin && u && input_ids && replaced, "st_attn_sched_inputs: null pointer");
  ST_CHECK(n > 0 && max_len >= 1 && max_len <= Tcap, "st_attn_sched_inputs: need n > 0 and 1 <= max_len <= Tcap (got %d, %d)", max_len, Tcap);
  if (st_sched_init_outputs(caption, n, Tcap, input_ids, replaced, drawn, logp, reinterpret_cast<hipStream_t>(stream), "st_attn_sched_inputs"))
    return 1;
  if (max_len == 1) return 0;                      // slot 0 (<start>) is never replaced
  const MixSpec mix = {caption_T, Tcap, lens, coin, u, prob, inv_temperature, top_k, input_ids, replaced, drawn, logp};
  return attn_greedy_run(p, cnn_feature, n, max_len - 1, 0, workspace, workspace_bytes, nullptr, nullptr, stream, "st_attn_sched_inputs", nullptr,
                         &mix);
}

// ---- beam search (beam_search.py:45-97 driven by the test branch rnn_attn.py:77-94) --------------------------------
// Fixed (image, slot) rows b*W + w as in beam.py: every iteration is one set of launches over the B*W rows and the fringe
// selection runs on the device (st_beam_select), so the caller reads the records back once and replays the Node bookkeeping.
namespace {
// hist_ld > 0 (keep_paths): the two path buffers follow the plain plan, whose offsets and total stay as they are
// G > 1 (the diverse search): its B * G done flags follow the path buffers, whose offsets stay as they are
struct BPlan : AttnPrep { int n, k; size_t h[2], c[2], x, z, att2, logits, tp, ti, gidx, slot, done, alpha, hist[2], done_g, total; };
BPlan make_bplan(const st_attn_params* p, int B, int W, int hist_ld, int G) {
  const st_rnn_params& r = p->rnn;
  const size_t es = st_dtype_size(r.dtype);
  BPlan q; Arena ar;
  const size_t n = (size_t)B * W;
  q.n = (int)n;
  q.k = W < r.V ? W : r.V;
  q.take_prep(ar, p, B);
  const size_t cs = r.cell == ST_CELL_LSTM ? (size_t)r.L * n * r.H * es : 0;
  for (int i = 0; i < 2; ++i) { q.h[i] = ar.take((size_t)r.L * n * r.H * es); q.c[i] = ar.take(cs); }
  q.x = ar.take(n * 2 * r.E * es); q.z = ar.take(n * p->F * es);
  q.att2 = ar.take(n * p->A * sizeof(float));
  q.logits = ar.take(n * st_up8(r.V) * sizeof(float));
  q.tp = ar.take(n * q.k * sizeof(float)); q.ti = ar.take(n * q.k * sizeof(long));
  q.gidx = ar.take(n * sizeof(int)); q.slot = ar.take(n * sizeof(int)); q.done = ar.take((size_t)B);
  q.alpha = ar.take(n * p->P * sizeof(float));
  for (int i = 0; i < 2; ++i) q.hist[i] = hist_ld > 0 ? ar.take(n * hist_ld * sizeof(int)) : 0;
  q.done_g = G > 1 ? ar.take((size_t)B * G) : q.done;
  q.total = ar.o;
  return q;
}

// st_beam_opts with the defaults of a NULL pointer: the plain search
st_beam_opts beam_opts(const st_beam_opts* o) { return o ? *o : st_beam_opts{0, 0, nullptr, 0, 0, 1, 0.f}; }

// slot (b, w) <- image b; fringe 0 = the roots alone: the first slot of every group of Wg slots (Wg = W with one group) holds
// start_id at cost 0, the others are empty (cost +inf); one done flag per (image, group)
// (hist0, nullable: every row's path starts with start_id)
__global__ void beam_seed_kernel(int B, int W, int Wg, long start_id, int* __restrict__ slot, long* __restrict__ tok0,
                                 float* __restrict__ cost0, int* __restrict__ par0, uint8_t* __restrict__ done, int* __restrict__ hist0,
                                 int hist_ld) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B * W) {
    if (hist0) hist0[(long)i * hist_ld] = (int)start_id;
    const bool root = (i % W) % Wg == 0;
    slot[i] = i / W;
    tok0[i] = root ? start_id : 0;
    cost0[i] = root ? 0.f : INFINITY;
    par0[i] = -1;
  }
  if (i < B * (W / Wg)) done[i] = 0;
}
}  // namespace

extern "C" size_t st_attn_beam_workspace_bytes(const st_attn_params* p, int B, int W, int max_length, const st_beam_opts* opts,
                                               size_t* last_paths_offset) {
  const st_beam_opts o = beam_opts(opts);
  if (last_paths_offset) *last_paths_offset = 0;
  if (!p || B <= 0 || W < 1 || W > 8 || max_length < 1 || o.num_groups < 1 || W % o.num_groups != 0 || !layers_ok(p)) return 0;
  if (o.keep_paths && max_length + 1 > ST_BEAM_MAX_HIST) return 0;
  const BPlan q = make_bplan(p, B, W, o.keep_paths ? max_length + 1 : 0, o.num_groups);
  if (last_paths_offset && o.keep_paths) *last_paths_offset = q.hist[max_length & 1];
  return q.total;
}

extern "C" int st_attn_beam_search(const st_attn_params* p, const float* cnn_feature, int B, int W, int max_length,
                                   long start_id, long end_id, void* workspace, size_t workspace_bytes,
                                   long* rec_tok, float* rec_cost, int* rec_par, uint8_t* rec_end, float* rec_alpha,
                                   const st_beam_opts* opts, void* stream) {
  if (check_common(p, nullptr, "st_attn_beam_search")) return 1;
  ST_CHECK(cnn_feature && workspace && rec_tok && rec_cost && rec_par && rec_end && B > 0, "st_attn_beam_search: bad arguments");
  ST_CHECK(W >= 1 && W <= 8, "st_attn_beam_search: beam width must be 1..8 (got %d)", W);
  ST_CHECK(max_length >= 1, "st_attn_beam_search: max_length must be >= 1 (got %d)", max_length);
  const st_rnn_params& r = p->rnn;
  ST_CHECK(r.w_lin && r.b_lin, "st_attn_beam_search: null vocabulary projection");
  const st_beam_opts o = beam_opts(opts);
  ST_CHECK(o.min_length >= 0, "st_attn_beam_search: min_length must be >= 0 (got %d)", o.min_length);
  ST_CHECK(o.ngram >= 0 && o.ngram <= ST_BEAM_MAX_NGRAM, "st_attn_beam_search: no_repeat_ngram_size must be 0..%d (got %d)", ST_BEAM_MAX_NGRAM, o.ngram);
  ST_CHECK(o.n_suppress >= 0 && o.n_suppress <= ST_BEAM_MAX_SUPPRESS && (o.n_suppress == 0 || o.suppress),
           "st_attn_beam_search: at most %d suppressed tokens (got %d)", ST_BEAM_MAX_SUPPRESS, o.n_suppress);
  ST_CHECK(!o.keep_paths || max_length + 1 <= ST_BEAM_MAX_HIST, "st_attn_beam_search: keeping the paths needs max_length + 1 <= %d (got %d)",
           ST_BEAM_MAX_HIST, max_length + 1);
  ST_CHECK(o.ngram == 0 || o.keep_paths, "st_attn_beam_search: n-gram blocking needs keep_paths");
  ST_CHECK(o.num_groups >= 1 && W % o.num_groups == 0, "st_attn_beam_search: the %d slots do not split into %d groups", W, o.num_groups);
  ST_CHECK(o.diversity_penalty >= 0.f && o.diversity_penalty < INFINITY, "st_attn_beam_search: diversity_penalty must be finite and >= 0 (got %g)",
           (double)o.diversity_penalty);
  // the ban kernel runs iff there is something to ban; an empty ban set gives st_softmax_topk's bits
  const bool bans = o.min_length > 0 || o.ngram > 0 || o.n_suppress > 0;
  ST_CHECK(!bans || r.V <= ST_BEAM_MAX_VOCAB, "st_attn_beam_search: V=%d exceeds the ban bitmap's %d entries", r.V, ST_BEAM_MAX_VOCAB);
  const int hist_ld = o.keep_paths ? max_length + 1 : 0, G = o.num_groups;
  const BPlan q = make_bplan(p, B, W, hist_ld, G);
  ST_CHECK(workspace_bytes >= q.total, "st_attn_beam_search: workspace too small (%zu < %zu)", workspace_bytes, q.total);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* ws = reinterpret_cast<char*>(workspace);
  const int dt = r.dtype, H = r.H, E = r.E, L = r.L, P = p->P, A = p->A, F = p->F, Vp = st_up8(r.V), n = q.n, k = q.k;
  const size_t es = st_dtype_size(dt);
  const bool lstm = r.cell == ST_CELL_LSTM;
  int* slot = reinterpret_cast<int*>(ws + q.slot);
  int* gidx = reinterpret_cast<int*>(ws + q.gidx);
  uint8_t* done = reinterpret_cast<uint8_t*>(ws + q.done_g);
  float* att2 = reinterpret_cast<float*>(ws + q.att2);
  float* logits = reinterpret_cast<float*>(ws + q.logits);
  float* tp = reinterpret_cast<float*>(ws + q.tp);
  long* ti = reinterpret_cast<long*>(ws + q.ti);

  if (prepare(p, cnn_feature, B, ws, q, stream)) return 1;
  int* hist[2] = {reinterpret_cast<int*>(ws + q.hist[0]), reinterpret_cast<int*>(ws + q.hist[1])};
  hipLaunchKernelGGL(beam_seed_kernel, dim3((n + 255) / 256), dim3(256), 0, st, B, W, W / G, start_id, slot, rec_tok, rec_cost, rec_par, done,
                     hist_ld ? hist[0] : nullptr, hist_ld);
  ST_LAUNCH_CHECK();
  // h0 (c0) repeated over the layers (rnn_attn.py:62), then scattered to the slots of its image
  if (replicate_rows_launch(ws + q.h0, ws + q.h[1], (long)B * H, L, dt, st)) return 1;
  if (st_gather_state(ws + q.h[1], slot, ws + q.h[0], L, B, n, H, dt, stream)) return 1;
  if (lstm) {
    if (replicate_rows_launch(ws + q.c0, ws + q.c[1], (long)B * H, L, dt, st)) return 1;
    if (st_gather_state(ws + q.c[1], slot, ws + q.c[0], L, B, n, H, dt, stream)) return 1;
  }
  for (int t = 0; t < max_length; ++t) {                                                   // beam_search.py:69
    const long* tok = rec_tok + (size_t)t * n;
    const float* cost = rec_cost + (size_t)t * n;
    const char* htop = ws + q.h[0] + (size_t)(L - 1) * n * H * es;                           // keyed on the previous top-layer state
    float* alpha_t = rec_alpha ? rec_alpha + (size_t)t * n * P : reinterpret_cast<float*>(ws + q.alpha);
    if (st_embedding_rows(r.emb, tok, ws + q.x, n, E, r.V, 2 * E, dt, stream)) return 1;
    if (skinny(htop, H, p->w_dec, H, att2, A, n, A, H, p->b_dec, 0, dt, st)) return 1;
    if (attn_beam_fwd_launch(ws + q.att1, att2, p->w_full, p->b_full, ws + q.feat, alpha_t, ws + q.z, B, W, P, A, F, dt, st)) return 1;
    if (skinny(ws + q.z, F, p->w_embed, F, ws + q.x + (size_t)E * es, 2 * E, n, E, F, p->b_embed, 0, dt, st, true)) return 1;
    if (st_rnn_step(&r, ws + q.x, n, ws + q.h[0], lstm ? ws + q.c[0] : nullptr, ws + q.h[1], lstm ? ws + q.c[1] : nullptr, logits, Vp, stream)) return 1;
    long* ntok = rec_tok + (size_t)(t + 1) * n;
    float* ncost = rec_cost + (size_t)(t + 1) * n;
    int* npar = rec_par + (size_t)(t + 1) * n;
    uint8_t* end_t = rec_end + (size_t)t * n;
    if (!bans) {
      if (st_softmax_topk(logits, Vp, n, r.V, k, tp, ti, 0, stream)) return 1;
    } else if (st_beam_ban_topk(logits, Vp, n, r.V, k, hist_ld ? hist[t & 1] : nullptr, hist_ld, t + 1, o.ngram, o.suppress, o.n_suppress,
                                end_id, t < o.min_length, tp, ti, stream)) return 1;       // the path of fringe t has t + 1 tokens
    if (st_beam_select(tok, cost, done, tp, ti, B, W, G, k, end_id, o.diversity_penalty, ntok, ncost, npar, end_t, gidx,
                       hist_ld ? hist[t & 1] : nullptr, hist_ld ? hist[(t + 1) & 1] : nullptr, hist_ld, t + 1, stream)) return 1;
    if (st_gather_state(ws + q.h[1], gidx, ws + q.h[0], L, n, n, H, dt, stream)) return 1;   // a child inherits its parent's state
    if (lstm && st_gather_state(ws + q.c[1], gidx, ws + q.c[0], L, n, n, H, dt, stream)) return 1;
  }
  return 0;
}
