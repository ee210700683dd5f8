// Teacher-forced decoder (GRU / LSTM over a packed sequence): forward and BPTT backward,
// each as ONE C-ABI call that issues every kernel of the pass on one stream.
//
// Replaces RNN.forward (reference rnn.py:27-35, LSTM/rnn_lstm.py:25-33) and the autograd
// backward torch builds for it (main.py:151).  Rows are time-major packed exactly as
// pack_padded_sequence orders them: row(t, b) = step_off[t] + b for b < batch_sizes[t].
//
// Both passes walk the (layer, time) grid by DIAGONALS: cell (l, t) needs (l-1, t) and (l, t-1) [forward] or
// (l+1, t) and (l, t+1) [backward], so the cells with l + t = d are independent and go out as ONE launch
// (blockIdx.z = cell).  A 5-layer, 18-step caption batch is 22 dependent launches instead of 90: the recurrence
// is launch-latency bound (a cell is ~0.2 GFLOP), so the count of dependent launches is what it costs.
//
// forward:  x0 = [feat ; emb(caption)] gathered straight into packed rows (no cat/pack copies)
//           per diagonal one fused launch: x W_ih^T + h W_hh^T + gates for every cell -> st_rnn_forward
//           logits = y_top W_lin^T + b
// backward: dlogits -> dW_lin, db_lin, dy_top; per diagonal (reversed) ONE fused launch in the pull form: cell (l, t) computes
//           dh = [dy_top] + dgh_{l,t+1} W_hh_l + dgx_{l+1,t} W_ih_{l+1} + its dh z carry from what the diagonal above wrote and
//           does its gate gradients in the epilogue (22 dependent launches, no fp32 dy round trip below the top layer);
//           dx0 = dgx_0 W_ih_0 is one whole-sequence GEMM after the wavefront; then every weight gradient (dW_lin, dW_ih_l, dW_hh_l)
//           with its bias gradient in grouped token-contraction launches that read the operands as they lie (bf16: st_gemm_tn_batch;
//           fp32 and ST_WGRAD_TN=0: K-major copies from transposes that also sum the bias gradients, then MFMA GEMMs).  ST_BPTT_FUSED=0 keeps the
//           earlier push route (a gate-gradient launch and a skinny-GEMM launch per diagonal)
//           -> st_rnn_backward
// dropout:  the entry points take an st_dropout (NULL or every p = 0: the plain call, launch for launch).  The input rows and the
//           rows in front of `linear` are masked outside the recurrence (st_dropout_rows: x0 in place, y_top into the caller's buffer,
//           and on the way back the fp32 dy_top and dx0 in place); the inter-layer site of nn.GRU(dropout=p) rides in the wavefront's
//           own launches (the DROP forms of the cell kernels): layer l writes h' for its recurrence and the dropped h' for layer l + 1,
//           and the BPTT cell masks the from-above product in registers.  dW_ih_{l+1} and dW_lin read the dropped copies, dW_hh_l the
//           plain rows.  With inter-layer dropout the backward pass is the fused route whatever ST_BPTT_FUSED says.
#include "decoder_host.h"
#include <stdlib.h>

namespace {

struct Plan {
  int G, GH, Np, Vp, maxw;
  size_t es;
  size_t x0, y, gates, cst, dyl, dx0, dgx, dgh, dhc, dcc, tA, tB, wT, wThh, wTih, gA, gB, total;
};

Plan make_plan(const st_rnn_params* p, const st_packed_seq* s) {
  Plan q;
  q.G = p->cell == ST_CELL_GRU ? 3 : 4;
  q.GH = q.G * p->H;
  q.Np = st_up8(s->ntok);
  q.Vp = st_rnn_vocab_ld(p->V);
  q.es = st_dtype_size(p->dtype);
  q.maxw = p->in0 > p->H ? p->in0 : p->H;
  const size_t n = s->ntok, L = p->L, H = p->H;
  Arena ar;
  q.x0 = ar.take(n * p->in0 * q.es);
  q.y = ar.take(L * n * H * q.es);
  q.gates = ar.take(L * n * 4 * H * q.es);
  q.cst = ar.take(p->cell == ST_CELL_LSTM ? L * n * H * q.es : 0);
  q.dyl = ar.take(L * n * H * sizeof(float));          // d loss / d y_l, one [ntok][H] fp32 matrix per layer
  q.dx0 = ar.take(n * p->in0 * sizeof(float));         // d loss / d x0
  q.dgx = ar.take(L * n * q.GH * q.es);                // gate gradients of every layer (operands of the dW GEMMs)
  q.dgh = ar.take(p->cell == ST_CELL_GRU ? L * n * q.GH * q.es : 0);
  q.dhc = ar.take(L * (size_t)s->B * H * sizeof(float));
  q.dcc = ar.take(L * (size_t)s->B * H * sizeof(float));
  // transposed operands: tA <= max(V, GH) x Np ; tB <= max(H, in0) x Np ; wT <= max(H x Vp, maxw x GH)
  const size_t ra = (size_t)(p->V > q.GH ? p->V : q.GH);
  q.tA = ar.take(ra * q.Np * q.es);
  q.tB = ar.take((size_t)q.maxw * q.Np * q.es);
  const size_t w1 = (size_t)H * q.Vp, w2 = (size_t)q.maxw * q.GH;
  q.wT = ar.take((w1 > w2 ? w1 : w2) * q.es);
  q.wThh = ar.take(L * H * q.GH * q.es);               // W_hh^T and W_ih^T of every layer: the backward wavefront needs them all
  q.wTih = ar.take(L * (size_t)q.maxw * q.GH * q.es);
  // K-major operands of the 2L weight-gradient GEMMs (dgx^T, x^T, dgh^T, hprev^T of every layer), alive together so that
  // the GEMMs can go out as one grouped launch
  q.gA = ar.take(2 * L * (size_t)q.GH * q.Np * q.es);
  q.gB = ar.take(2 * L * (size_t)q.maxw * q.Np * q.es);
  q.total = ar.o;
  return q;
}

int check_common(const st_rnn_params* p, const st_packed_seq* s, const char* who) {
  ST_CHECK(p && s, "%s: null descriptor", who);
  ST_CHECK(p->cell == ST_CELL_GRU || p->cell == ST_CELL_LSTM, "%s: bad cell %d", who, p->cell);
  ST_CHECK(p->dtype == ST_F32 || p->dtype == ST_BF16, "%s: bad dtype %d", who, p->dtype);
  ST_CHECK(p->L >= 1 && p->L <= ST_MAX_LAYERS, "%s: num_layers=%d out of range [1,%d]", who, p->L, ST_MAX_LAYERS);
  ST_CHECK(p->H % 8 == 0 && p->in0 % 8 == 0 && p->E % 8 == 0, "%s: E=%d, in0=%d and H=%d must be multiples of 8", who, p->E, p->in0, p->H);
  ST_CHECK(p->V > 0, "%s: bad vocabulary size", who);
  if (st_check_packed_seq(s, who, true)) return 1;
  for (int l = 0; l < p->L; ++l)
    ST_CHECK(p->w_ih[l] && p->w_hh[l] && p->b_ih[l] && p->b_hh[l], "%s: null weights for layer %d", who, l);
  return 0;
}

}  // namespace

// Leading dimension to give logits / dlogits rows: V rounded up to 8 elements for small vocabularies, to 512 (8 K tiles of
// 64) from 2048 entries on, so that the K = V product of the backward pass can be split evenly.
extern "C" int st_rnn_vocab_ld(int V) { return V < 2048 ? st_up8(V) : (V + 511) / 512 * 512; }

extern "C" size_t st_rnn_workspace_bytes(const st_rnn_params* p, const st_packed_seq* s) {
  if (!p || !s || p->L < 1 || p->L > ST_MAX_LAYERS) return 0;   // 0: no entry point accepts this descriptor
  return make_plan(p, s).total;
}

// input_ids [B][Tcap] (NULL: s->caption): what the layer-0 rows t >= 1 embed, apart from the targets (scheduled sampling)
extern "C" int st_rnn_forward(const st_rnn_params* p, const st_packed_seq* s, const void* feat,
                              void* workspace, size_t workspace_bytes, void* logits, int logits_dtype, int ldl,
                              long* targets, int save_for_backward, const st_dropout* drop, const long* input_ids, void* stream) {
  if (check_common(p, s, "st_rnn_forward")) return 1;
  ST_CHECK(p->in0 == p->E, "st_rnn_forward: in0=%d != E=%d (the layer-0 rows are [feature ; embeddings])", p->in0, p->E);
  DropPlan dp;
  if (st_drop_plan(drop, p->L, s->ntok, p->H, p->dtype, false, "st_rnn_forward", &dp)) return 1;
  ST_CHECK(workspace && feat && p->emb, "st_rnn_forward: null pointer");
  const Plan q = make_plan(p, s);
  ST_CHECK(workspace_bytes >= q.total, "st_rnn_forward: workspace too small (%zu < %zu)", workspace_bytes, q.total);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* ws = reinterpret_cast<char*>(workspace);
  const int dt = p->dtype, H = p->H, n = s->ntok;
  const size_t es = q.es;

  // input_ids: the rows t >= 1 gather emb[input_ids[b][t-1]]; the targets stay the caption's
  const char* x0 = ws + q.x0;
  if (pack_inputs_launch(feat, p->emb, s->caption, s->Tcap, s->rows_b, s->rows_t, ws + q.x0, targets, n, p->E, p->V, 0, dt, st, input_ids)) return 1;
  if (dp.in && dropout_rows_launch(x0, ws + q.x0, dt, n, p->in0, p->in0, p->in0, dp.kin, kDropSiteInput, 0, st)) return 1;
  const std::vector<int> off = st_packed_offsets(s);

  const int L = p->L, T = s->T;
  for (int d = 0; d < T + L - 1; ++d) {
    RnnGemmArgs cells[ST_MAX_LAYERS];
    RnnDropArgs da;
    memset(&da, 0, sizeof(da));
    da.key = dp.klayer;
    int nc = 0;
    for (int l = d < T ? 0 : d - (T - 1); l <= d && l < L; ++l) {
      const int t = d - l;
      const int bt = s->batch_sizes_host[t];
      // with inter-layer dropout layer l reads the dropped copy of y_{l-1}; the recurrence keeps the plain rows
      const char* xl = l == 0 ? x0 : dp.layer ? dp.rows(l - 1) : ws + q.y + (size_t)(l - 1) * n * H * es;
      const int in = l == 0 ? p->in0 : H;
      char* yl = ws + q.y + (size_t)l * n * H * es;
      char* gl = ws + q.gates + (size_t)l * n * 4 * H * es;
      char* cl = ws + q.cst + (size_t)l * n * H * es;
      cells[nc++] = rnn_full_cell(p, l, xl + (size_t)off[t] * in * es, in, t > 0 ? yl + (size_t)off[t - 1] * H * es : nullptr,
                                  t > 0 ? cl + (size_t)off[t - 1] * H * es : nullptr, yl + (size_t)off[t] * H * es, cl + (size_t)off[t] * H * es,
                                  bt, save_for_backward ? gl + (size_t)off[t] * 4 * H * es : nullptr);
      if (dp.layer) {
        if (l + 1 < L) { cells[nc - 1].hout2 = dp.rows(l) + (size_t)off[t] * H * es; cells[nc - 1].ldho2 = H; }
        da.site[nc - 1] = l; da.row0[nc - 1] = off[t];
      }
    }
    if (dp.layer ? rnn_gemm_launch_batch_drop(cells, nc, dt, rnn_cell_epi(p->cell), da, st)
                 : rnn_gemm_launch_batch(cells, nc, dt, rnn_cell_epi(p->cell), 1, st)) return 1;
  }
  const char* ytop = ws + q.y + (size_t)(p->L - 1) * n * H * es;
  if (dp.out) {                                    // Dropout in front of `linear`: the projection and dW_lin read the dropped copy
    if (dropout_rows_launch(ytop, dp.rows(L - 1), dt, n, H, H, H, dp.kout, L - 1, 0, st)) return 1;
    ytop = dp.rows(L - 1);
  }
  if (logits) {
    ST_CHECK(p->w_lin && p->b_lin, "st_rnn_forward: logits requested without the vocabulary projection");
    if (st_gemm_nt(ytop, H, p->w_lin, H, logits, ldl, n, p->V, H, dt, logits_dtype, p->b_lin, stream)) return 1;
  }
  return 0;
}
extern "C" size_t st_rnn_dropout_bytes(const st_rnn_params* p, const st_packed_seq* s) {
  if (!p || !s) return 0;
  return st_dropout_buf_bytes(p->L, s->ntok, p->H, p->dtype);
}

// ---- vocabulary projection + nn.CrossEntropyLoss() fused (csrc/vocab_ce.hip): the logits are never written ---------------------------------
// scratch (floats): lse[ntok] | target logit[ntok] | partial[ntok][tiles][2]; lse stays valid for st_rnn_fused_dlogits
extern "C" int st_rnn_fused_loss_supported(const st_rnn_params* p) {
  return p && p->w_lin && p->b_lin && vocab_ce_supported(p->dtype, p->H) ? 1 : 0;
}
extern "C" size_t st_rnn_fused_loss_bytes(const st_rnn_params* p, const st_packed_seq* s) {
  if (!p || !s) return 0;
  return ((size_t)s->ntok * (2 + 2 * (size_t)vocab_ce_tiles(p->V))) * sizeof(float);
}
// tile_sums of st_loss_terms (floats): [tiles][ntok] sums of each tile's valid logits, caller-owned so that st_rnn_fused_loss_bytes stays what it was
extern "C" size_t st_rnn_fused_loss_ls_bytes(const st_rnn_params* p, const st_packed_seq* s) {
  if (!p || !s) return 0;
  return (size_t)s->ntok * (size_t)vocab_ce_tiles(p->V) * sizeof(float);
}

namespace {
// What the loss and the dlogits call check alike, and the rows they hand to the vocabulary kernels: the dropped copy of y_top when
// drop->p_out > 0, else the workspace's
int fused_rows(const st_rnn_params* p, const st_packed_seq* s, const void* workspace, size_t workspace_bytes, const st_loss_terms* t,
               const st_dropout* drop, const char* who, const char** ytop) {
  if (check_common(p, s, who)) return 1;
  if (st_check_loss_terms(t, who)) return 1;
  ST_CHECK(st_rnn_fused_loss_supported(p), "%s: needs bf16, H = 512 and the vocabulary projection (use st_rnn_forward's logits + st_cross_entropy)", who);
  const Plan q = make_plan(p, s);
  ST_CHECK(workspace, "%s: null pointer", who);
  ST_CHECK(workspace_bytes >= q.total, "%s: workspace / scratch too small", who);
  DropPlan dp;
  if (st_drop_plan(drop, p->L, s->ntok, p->H, p->dtype, false, who, &dp)) return 1;
  *ytop = dp.out ? dp.rows(p->L - 1) : reinterpret_cast<const char*>(workspace) + q.y + (size_t)(p->L - 1) * s->ntok * p->H * q.es;
  return 0;
}
}  // namespace

// *loss_accum += sum_r row_weight[r] * ((1 - eps) * nll_r + eps * u_r) / ntok over the rows `linear` reads (terms: st_loss_terms, NULL = the
// plain mean); smoothing = 0 runs the kernels without the tile sums, smoothing = 1 the label-smoothing ones at any eps in [0, 1)
extern "C" int st_rnn_fused_loss(const st_rnn_params* p, const st_packed_seq* s, const void* workspace, size_t workspace_bytes,
                                 const long* targets, float* scratch, size_t scratch_bytes, const st_loss_terms* terms, float* loss_accum,
                                 const st_dropout* drop, void* stream) {
  const st_loss_terms t = terms ? *terms : st_loss_terms{};
  const char* ytop;
  if (fused_rows(p, s, workspace, workspace_bytes, &t, drop, "st_rnn_fused_loss", &ytop)) return 1;
  ST_CHECK(targets && scratch && (loss_accum || t.nll_out || t.smooth_out) && (t.tile_sums || !t.smoothing), "st_rnn_fused_loss: null pointer");
  ST_CHECK(scratch_bytes >= st_rnn_fused_loss_bytes(p, s), "st_rnn_fused_loss: workspace / scratch too small");
  ST_CHECK(!t.smoothing || t.tile_sums_bytes >= st_rnn_fused_loss_ls_bytes(p, s), "st_rnn_fused_loss: tile_sums too small (%zu < %zu)",
           t.tile_sums_bytes, st_rnn_fused_loss_ls_bytes(p, s));
  const int n = s->ntok;
  // smoothing = 0: tile_sums, smooth_out and label_smoothing are NULL, NULL and 0 (checked), which is vocab_ce_forward without them
  return vocab_ce_forward(ytop, p->w_lin, p->b_lin, targets, n, p->V, scratch + 2 * (size_t)n, scratch + n, scratch, loss_accum, t.row_weight,
                          t.nll_out, reinterpret_cast<hipStream_t>(stream), t.tile_sums, t.smooth_out, t.label_smoothing);
}
// dlogits[ntok][ldd] (bf16) = (softmax - (1 - eps) * onehot - eps / V) / ntok * *grad_scale_dev (* row_weight[r]) from the same tile
// products; pad columns [V, ldd) zero.  Reads row_weight, smoothing and label_smoothing of `terms`
extern "C" int st_rnn_fused_dlogits(const st_rnn_params* p, const st_packed_seq* s, const void* workspace, size_t workspace_bytes,
                                    const long* targets, const float* scratch, const float* grad_scale_dev, const st_loss_terms* terms,
                                    void* dlogits, int ldd, const st_dropout* drop, void* stream) {
  const st_loss_terms t = terms ? *terms : st_loss_terms{};
  const char* ytop;
  if (fused_rows(p, s, workspace, workspace_bytes, &t, drop, "st_rnn_fused_dlogits", &ytop)) return 1;
  ST_CHECK(targets && scratch && dlogits, "st_rnn_fused_dlogits: null pointer");
  return vocab_ce_dlogits(ytop, p->w_lin, p->b_lin, targets, scratch, s->ntok, p->V, dlogits, ldd, 1.0f, grad_scale_dev, t.row_weight,
                          reinterpret_cast<hipStream_t>(stream), t.smoothing != 0, t.label_smoothing);
}

// after st_rnn_forward with the same `drop` (its buffer holds the dropped copies the weight gradients read) and the same input_ids (the
// embedding gradient scatters to the tokens that were fed)
extern "C" int st_rnn_backward(const st_rnn_params* p, const st_rnn_grads* g, const st_packed_seq* s, const void* dlogits, int ldd,
                               void* workspace, size_t workspace_bytes, float* dfeat, const st_dropout* drop, const long* input_ids,
                               void* stream) {
  if (check_common(p, s, "st_rnn_backward")) return 1;
  ST_CHECK(g && workspace && dlogits, "st_rnn_backward: null pointer");
  DropPlan dp;
  if (st_drop_plan(drop, p->L, s->ntok, p->H, p->dtype, false, "st_rnn_backward", &dp)) return 1;
  const Plan q = make_plan(p, s);
  ST_CHECK(workspace_bytes >= q.total, "st_rnn_backward: workspace too small (%zu < %zu)", workspace_bytes, q.total);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* ws = reinterpret_cast<char*>(workspace);
  const int dt = p->dtype, H = p->H, n = s->ntok, Np = q.Np, GH = q.GH;
  const size_t es = q.es;
  const std::vector<int> off = st_packed_offsets(s);
  const int L = p->L, T = s->T;
  auto dyl = [&](int l) { return reinterpret_cast<float*>(ws + q.dyl) + (size_t)l * n * H; };   // d loss / d y_l
  float* dy = dyl(L - 1);
  const char* ytop = dp.out ? dp.rows(L - 1) : ws + q.y + (size_t)(p->L - 1) * n * H * es;   // what `linear` read

  // bf16: every weight gradient (and the bias gradient that goes with it) is a token contraction of operands read as they lie
  // (st_gemm_tn_batch, csrc/gemm_tn.hip), collected here and sent as grouped launches after the wavefront.  ST_WGRAD_TN=0 (read per
  // call: A/B runs, tests) keeps the K-major copies and st_gemm_nt, which is also what fp32 runs (the transposed LDS read is a
  // 16-bit one).  The regions tA, tB, gA and gB of the workspace stay reserved for that route.
  const char* env_tn = getenv("ST_WGRAD_TN");
  const bool tn = dt == ST_BF16 && !(env_tn && env_tn[0] == '0');
  st_gemm_tn_desc tg[2 * ST_MAX_LAYERS + 1];
  int ntg = 0;
  auto tn_desc = [&](const void* a, int lda, const void* b, int ldb, float* c, int rows, int cols, float* cs0, float* cs1, bool hprev) {
    st_gemm_tn_desc d;                             // c[rows][cols] += a[n][rows]^T b[n][cols]
    memset(&d, 0, sizeof(d));
    d.a = a; d.b = b; d.c = c; d.colsum0 = cs0; d.colsum1 = cs1; d.dtype = dt;
    d.M = rows; d.N = cols; d.K = n; d.lda = lda; d.ldb = ldb; d.ldc = cols; d.accumulate = 1;
    if (hprev) { d.b_row = s->prev_row; d.b_live = s->rows_t; }   // row r of b is y[prev_row[r]], zero at t = 0
    return d;
  };

  ST_CHECK(p->w_lin && g->w_lin && g->b_lin, "st_rnn_backward: vocabulary projection gradients requested without buffers");
  ST_CHECK(ldd >= st_up8(p->V) && ldd % 8 == 0 && ldd <= q.Vp, "st_rnn_backward: dlogits leading dimension %d must be a multiple of 8 in [%d, %d]",
           ldd, st_up8(p->V), q.Vp);
  // db = colsum(dlogits);  dW_lin += dlogits^T y_top;  dy_top = dlogits W_lin
  if (tn) {                                      // contracted over the tokens as the operands lie, with the layers' gradients below
    tg[ntg++] = tn_desc(dlogits, ldd, ytop, H, g->w_lin, p->V, H, g->b_lin, nullptr, false);
  } else {
    if (st_transpose_colsum(dlogits, ws + q.tA, g->b_lin, dt, n, p->V, ldd, Np, stream)) return 1;
    if (st_transpose(ytop, ws + q.tB, dt, n, H, H, Np, stream)) return 1;
    if (st_gemm_nt(ws + q.tA, Np, ws + q.tB, Np, g->w_lin, H, p->V, H, Np, dt, ST_F32, nullptr, stream, 1)) return 1;
  }
  // dy = dlogits W_lin is 15 x 4 output tiles over K = V: with the padded leading dimension (st_rnn_vocab_ld: a multiple
  // of 8 K tiles, pad columns zero on both sides) it runs as 8 K slices in one grouped launch
  if (st_transpose(p->w_lin, ws + q.wT, dt, p->V, H, H, ldd, stream)) return 1;
  const int bk = dt == ST_BF16 ? 64 : 32;
  const int split = (ldd % (8 * bk) == 0 && ldd >= 16 * bk) ? 8 : 0;
  if (st_gemm_nt(dlogits, ldd, ws + q.wT, ldd, dy, H, n, H, ldd, dt, ST_F32, nullptr, stream, 0, split)) return 1;
  if (dp.out && dropout_rows_launch(dy, dy, ST_F32, n, H, H, H, dp.kout, L - 1, 0, st)) return 1;   // d dropped y_top -> d y_top

  const char* x0 = ws + q.x0;
  const bool need_dx0 = dfeat || g->emb;
  float* dx0 = reinterpret_cast<float*>(ws + q.dx0);
  const bool gru = p->cell == ST_CELL_GRU;
  auto dgxl = [&](int l) { return ws + q.dgx + (size_t)l * n * GH * es; };
  auto dghl = [&](int l) { return gru ? ws + q.dgh + (size_t)l * n * GH * es : dgxl(l); };   // LSTM: one gradient feeds both projections
  auto dhcl = [&](int l) { return reinterpret_cast<float*>(ws + q.dhc) + (size_t)l * s->B * H; };
  auto dccl = [&](int l) { return reinterpret_cast<float*>(ws + q.dcc) + (size_t)l * s->B * H; };
  auto wThh = [&](int l) { return ws + q.wThh + (size_t)l * H * GH * es; };
  auto wTih = [&](int l) { return ws + q.wTih + (size_t)l * q.maxw * GH * es; };
  if (hipMemsetAsync(ws + q.dhc, 0, (size_t)L * s->B * H * sizeof(float), st) != hipSuccess ||
      hipMemsetAsync(ws + q.dcc, 0, (size_t)L * s->B * H * sizeof(float), st) != hipSuccess) { st_set_error("memset failed"); return 1; }
  {   // K-major operands of dh_{t-1} += dgh_t W_hh  and  dx_t = dgx_t W_ih: one batched transpose per kind
    const void* wx[2][ST_MAX_LAYERS]; void* wy[2][ST_MAX_LAYERS];
    int ni = 0;
    for (int l = 0; l < L; ++l) {
      const int in = l == 0 ? p->in0 : H;
      wx[0][l] = p->w_hh[l]; wy[0][l] = wThh(l);
      if (!(l > 0 || need_dx0)) continue;
      if (in == H) { wx[1][ni] = p->w_ih[l]; wy[1][ni] = wTih(l); ++ni; }
      else if (st_transpose(p->w_ih[l], wTih(l), dt, GH, in, in, GH, stream)) return 1;
    }
    if (st_transpose_batch(wx[0], wy[0], nullptr, L, dt, GH, H, H, GH, nullptr, nullptr, stream)) return 1;
    if (ni && st_transpose_batch(wx[1], wy[1], nullptr, ni, dt, GH, H, H, GH, nullptr, nullptr, stream)) return 1;
  }
  auto bwd_cell = [&](int l, int t, const float* dyrows) {   // gate gradients of cell (l, t); dyrows: d loss / d y_l from row 0 on, or NULL
    const char* yl = ws + q.y + (size_t)l * n * H * es;
    const char* gl = ws + q.gates + (size_t)l * n * 4 * H * es;
    const char* cl = ws + q.cst + (size_t)l * n * H * es;
    RnnBwdCell c;
    memset(&c, 0, sizeof(c));
    c.dy = dyrows ? dyrows + (size_t)off[t] * H : nullptr; c.dhc = dhcl(l); c.dcc = dccl(l);
    c.cache = gl + (size_t)off[t] * 4 * H * es;
    c.hprev = t > 0 ? yl + (size_t)off[t - 1] * H * es : nullptr;
    c.cnew = cl + (size_t)off[t] * H * es;
    c.cprev = t > 0 ? cl + (size_t)off[t - 1] * H * es : nullptr;
    c.dgx = dgxl(l) + (size_t)off[t] * GH * es; c.dgh = dghl(l) + (size_t)off[t] * GH * es; c.Bt = s->batch_sizes_host[t];
    return c;
  };
  // reversed wavefront: the cells of a diagonal need only cells of the diagonal above
  const char* env = getenv("ST_BPTT_FUSED");       // read per call: ST_BPTT_FUSED=0 keeps the two-launch push route (A/B runs, tests)
  const bool fused = !(env && env[0] == '0') || dp.layer;   // the inter-layer mask lives in the fused cell only
  // pull form, one launch per diagonal: cell (l, t) takes dgh_{l,t+1} W_hh_l and dgx_{l+1,t} W_ih_{l+1} from what the diagonal
  // above wrote, adds dy (top layer) and its own dh z carry, and does its gate gradients in the epilogue
  for (int d = T + L - 2; fused && d >= 0; --d) {
    RnnBwdFused fc[ST_MAX_LAYERS];
    RnnDropArgs da;
    memset(&da, 0, sizeof(da));
    da.key = dp.klayer;
    int nf = 0;
    for (int l = d < T ? 0 : d - (T - 1); l <= d && l < L; ++l) {
      const int t = d - l;
      RnnBwdFused& f = fc[nf++];
      memset(&f, 0, sizeof(f));
      f.e = bwd_cell(l, t, l == L - 1 ? dy : nullptr);
      da.site[nf - 1] = l; da.row0[nf - 1] = off[t];
      RnnGemmArgs& a = f.g;
      a.M = f.e.Bt; a.N = H;
      if (t + 1 < T) {                             // rows [B_{t+1}, B_t) end here: no recurrent term
        a.A = dghl(l) + (size_t)off[t + 1] * GH * es; a.W = wThh(l); a.M2 = s->batch_sizes_host[t + 1]; a.K = GH; a.lda = GH; a.ldw = GH;
      }
      if (l + 1 < L) {
        a.A2 = dgxl(l + 1) + (size_t)off[t] * GH * es; a.W2 = wTih(l + 1); a.K2 = GH; a.lda2 = GH; a.ldw2 = GH;
      }
    }
    if (dp.layer ? rnn_bwd_fused_launch_batch_drop(fc, nf, p->cell, dt, da, st) : rnn_bwd_fused_launch_batch(fc, nf, p->cell, dt, st)) return 1;
  }
  // dx0 = dgx_0 W_ih_0 feeds only the embedding / feature gradients: one whole-sequence GEMM off the recurrence
  if (fused && need_dx0 && st_gemm_nt(dgxl(0), GH, wTih(0), GH, dx0, p->in0, n, p->in0, GH, dt, ST_F32, nullptr, stream)) return 1;
  for (int d = T + L - 2; !fused && d >= 0; --d) {
    RnnBwdCell gc[ST_MAX_LAYERS];
    RnnGemmArgs mc[2 * ST_MAX_LAYERS];
    int ng = 0, nm = 0;
    for (int l = d < T ? 0 : d - (T - 1); l <= d && l < L; ++l) {
      const int t = d - l;
      const int bt = s->batch_sizes_host[t];
      const int in = l == 0 ? p->in0 : H;
      gc[ng++] = bwd_cell(l, t, dyl(l));
      if (t > 0) {                                 // dh_{t-1} += dgh_t W_hh
        RnnGemmArgs& a = mc[nm++];
        memset(&a, 0, sizeof(a));
        a.A = dghl(l) + (size_t)off[t] * GH * es; a.W = wThh(l); a.M = bt; a.N = H; a.K = GH; a.lda = GH; a.ldw = GH;
        a.out_f32 = dhcl(l); a.ldo = H; a.accumulate = 1;
      }
      if (l > 0 || need_dx0) {                     // dx_t = dgx_t W_ih: the gradient the layer below reads at this step
        RnnGemmArgs& a = mc[nm++];
        memset(&a, 0, sizeof(a));
        a.A = dgxl(l) + (size_t)off[t] * GH * es; a.W = wTih(l); a.M = bt; a.N = in; a.K = GH; a.lda = GH; a.ldw = GH;
        a.out_f32 = (l > 0 ? dyl(l - 1) + (size_t)off[t] * H : dx0 + (size_t)off[t] * in); a.ldo = in;
      }
    }
    if (rnn_bwd_gates_launch_batch(gc, ng, H, p->cell, dt, st)) return 1;
    if (rnn_gemm_launch_batch(mc, nm, dt, 0, 0, st)) return 1;
  }
  // d dropped x0 -> d x0, before the embedding / feature gradients read it
  if (dp.in && need_dx0 && dropout_rows_launch(dx0, dx0, ST_F32, n, p->in0, p->in0, p->in0, dp.kin, kDropSiteInput, 0, st)) return 1;
  if (need_dx0) {
    ST_CHECK(g->emb, "st_rnn_backward: embedding gradient buffer missing");
    if (embedding_bwd_launch(dx0, input_ids ? input_ids : s->caption, s->Tcap, s->rows_b, s->rows_t, dfeat, g->emb, n, p->E, p->V, 0, st)) return 1;
  }
  // parameter gradients, bf16: dW_ih_l += dgx_l^T x_l and dW_hh_l += dgh_l^T h_{t-1} (y_l gathered through prev_row) with their bias
  // gradients as column sums, one group each beside dW_lin's; a layer whose input width is not H is a group like the others
  for (int l = 0; tn && l < L; ++l) {
    const int in = l == 0 ? p->in0 : H;
    // dW_ih_l contracts with what layer l READ: the dropped copy of y_{l-1} (x0 was dropped in place); dW_hh_l with the plain y_l
    const char* xl = l == 0 ? x0 : dp.layer ? dp.rows(l - 1) : ws + q.y + (size_t)(l - 1) * n * H * es;
    // LSTM: dgh == dgx, so its column sums are both bias gradients and the recurrent group adds none
    tg[ntg++] = tn_desc(dgxl(l), GH, xl, in, g->w_ih[l], GH, in, g->b_ih[l], gru ? nullptr : g->b_hh[l], false);
    tg[ntg++] = tn_desc(dghl(l), GH, ws + q.y + (size_t)l * n * H * es, H, g->w_hh[l], GH, H, gru ? g->b_hh[l] : nullptr, nullptr, true);
  }
  for (int i = 0; i < ntg; i += 12) {
    if (st_gemm_tn_batch(tg + i, ntg - i < 12 ? ntg - i : 12, stream)) return 1;
  }
  if (tn) return 0;
  // parameter gradients: K-major copies of every layer's operands (the transposes also sum the bias gradients), then the
  // 2L weight-gradient GEMMs -- 48 tiles each -- as grouped launches (st_conv_batch) that fill the chip
  st_conv_desc gd[2 * ST_MAX_LAYERS];
  int ng = 0;
  auto wgrad = [&](const void* aT, const void* bT, float* dw, int rows, int cols) {   // dw[rows][cols] += aT[rows][Np] . bT[cols][Np]^T
    gd[ng++] = st_gemm_nt_desc(aT, Np, bT, Np, dw, cols, rows, cols, Np, dt, ST_F32, nullptr, 1);
  };
  const void* tx[4][ST_MAX_LAYERS]; void* ty[4][ST_MAX_LAYERS]; float* tc[4][ST_MAX_LAYERS];   // dgx, x, dgh, y(->hprev) of every layer
  int nx = 0;                                                                                   // layers whose input width is H
  for (int l = 0; l < L; ++l) {
    const int in = l == 0 ? p->in0 : H;
    // dW_ih_l contracts with what layer l READ: the dropped copy of y_{l-1} (x0 was dropped in place); dW_hh_l with the plain y_l
    const char* xl = l == 0 ? x0 : dp.layer ? dp.rows(l - 1) : ws + q.y + (size_t)(l - 1) * n * H * es;
    char* aIh = ws + q.gA + (size_t)(2 * l) * GH * Np * es;
    char* aHh = ws + q.gA + (size_t)(2 * l + 1) * GH * Np * es;
    char* bIh = ws + q.gB + (size_t)(2 * l) * q.maxw * Np * es;
    char* bHh = ws + q.gB + (size_t)(2 * l + 1) * q.maxw * Np * es;
    tx[0][l] = dgxl(l); ty[0][l] = aIh; tc[0][l] = g->b_ih[l];
    tx[2][l] = dghl(l); ty[2][l] = aHh; tc[2][l] = g->b_hh[l];
    tx[3][l] = ws + q.y + (size_t)l * n * H * es; ty[3][l] = bHh; tc[3][l] = nullptr;
    if (in == H) {                       // same shape as the recurrent one: joins the groups
      tx[1][nx] = xl; ty[1][nx] = bIh; tc[1][nx] = nullptr; ++nx;
      wgrad(aIh, bIh, g->w_ih[l], GH, in);
    } else {
      if (st_transpose(xl, bIh, dt, n, in, in, Np, stream)) return 1;
    }
    wgrad(gru ? aHh : aIh, bHh, g->w_hh[l], GH, H);
    if (!gru && colsum_launch(dghl(l), g->b_hh[l], n, GH, GH, dt, st)) return 1;   // LSTM: dgh == dgx, transposed once
  }
  // one launch per operand kind over all layers; the bias gradients ride on the gate-gradient transposes and h_{t-1}
  // is gathered by the transpose itself (packed-sequence prev_row table)
  if (st_transpose_batch(tx[0], ty[0], tc[0], L, dt, n, GH, GH, Np, nullptr, nullptr, stream)) return 1;
  if (nx && st_transpose_batch(tx[1], ty[1], nullptr, nx, dt, n, H, H, Np, nullptr, nullptr, stream)) return 1;
  if (gru && st_transpose_batch(tx[2], ty[2], tc[2], L, dt, n, GH, GH, Np, nullptr, nullptr, stream)) return 1;
  if (st_transpose_batch(tx[3], ty[3], nullptr, L, dt, n, H, H, Np, s->rows_t, s->prev_row, stream)) return 1;
  for (int l = 0; l < L; ++l) {          // layers with a different input width: their dW_ih on its own
    const int in = l == 0 ? p->in0 : H;
    if (in != H && st_gemm_nt(ws + q.gA + (size_t)(2 * l) * GH * Np * es, Np, ws + q.gB + (size_t)(2 * l) * q.maxw * Np * es, Np,
                              g->w_ih[l], in, GH, in, Np, dt, ST_F32, nullptr, stream, 1)) return 1;
  }
  for (int i = 0; i < ng; i += 12) {
    if (st_conv_batch(gd + i, ng - i < 12 ? ng - i : 12, stream)) return 1;
  }
  return 0;
}
