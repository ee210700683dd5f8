"""Cases, inputs, launch arithmetic, storage replica and seeded faults for tests/test_gpu_decoder_geometry.py (GPU) and
tests/test_decoder_geometry_inputs.py (CPU): the plain GRU / LSTM decoders over widths, vocabularies and batch shapes.  Nothing here
needs a GPU.

  CASES            the case table: the smallest shapes at which E, H, V, B and L take each launch path of csrc/rnn.cpp,
                   csrc/rnn_kernels.hip, csrc/gemm_tn.hip, csrc/igemm.hip and csrc/decode.hip
  problem          (params, feat, cap, lens) of one (case, cell, dtype), bf16-representable for the bf16 kernels
  paths            pure-Python mirror of the launch arithmetic (make_plan, st_rnn_vocab_ld, the dy split, gemm_launch, skinny_mma's
                   K steps per wave, the gemm_tn tile grid, dispatch_kc's N <= 64 branch, vocab_argmax_launch, the fused
                   cross-entropy and pipelined-decoder eligibility)
  train_copy       R.gru_train_loss cell by cell, with bf16 rounding where st_rnn_forward stores (`storage`) and the seeded faults
  grads            float64 (loss, packed logits, {name: gradient, 'feat': gradient}) of the copy, cached
  storage_distance what bf16 storage alone does to each gradient; STORAGE_FLOORS is its record and bf16_bounds reads it
  greedy_walk      R.rnn_greedy / R.rnn_greedy_bf16_storage walked along given tokens; fp32_greedy_floor / FP32_GAP the gap a
                   fp32 token is compared beyond, plain_greedy_floor / GREEDY_LOOSE the bf16 rule of tests/_decoder_depth_cases.py
Every table of floors is recomputed by tests/test_decoder_geometry_inputs.py, which fails when a recorded figure is stale.
"""
import functools

import torch

from oracle import restatement as R
from tests import _attention_geometry_cases as G
from tests._decoder_depth_cases import captions, distance, pipe_eligible, token_logp  # noqa: F401  (the GPU test reads them from here)
from tests.test_gpu_decoder_bench_shape import (AGREE, DELTA, GRAD_L2, GRAD_MAX, ROW_L2, _bf16, _bf16_params, _greedy_bounds, _rel_l2,
                                                _rel_max)
from tests.test_gpu_rnn_bptt_fused import _lens_ragged

V = 50
STEPS = R.CAP_MAX


def _lens_tall():
    """B = 520, packed batch sizes 520, 513: both steps are a single cell of 512 rows or more; ntok = 1033"""
    lens = [2] * 513 + [1] * 7
    assert R.batch_sizes(lens) == [520, 513] and sum(lens) == 1033
    return lens


# `scale` (per cell) multiplies the recurrent weights (unit.weight_*), `lin` linear.weight, as tests/_decoder_depth_cases.py does and
# for its reason: a freshly initialised stack gives nearly the same top row to every token and nearly uniform logits, and then a lost
# tile or a dropped K tail moves nothing.  The values are the smallest at which the signal, power and greedy-gap conditions of
# test_decoder_geometry_inputs.py hold with room (figures there).
CASES = {
    #                        E      H    L   V     lens
    "e_wider": dict(E=72, H=24, L=2, V=12, lens=[4, 4, 3, 2, 2], seed=21, scale=dict(gru=2.0, lstm=3.0), lin=6.0),
    "h200": dict(E=200, H=200, L=2, V=V, lens=_lens_ragged(), seed=22, scale=dict(gru=2.0, lstm=3.0), lin=6.0),
    "h520": dict(E=520, H=520, L=2, V=V, lens=[3] * 5, seed=23, scale=dict(gru=2.0, lstm=3.0), lin=6.0),
    "h256": dict(E=256, H=256, L=1, V=V, lens=[2] * 33, seed=24, scale=dict(gru=2.0, lstm=3.0), lin=6.0),       # greedy only
    "v2047": dict(E=64, H=64, L=1, V=2047, lens=[3] * 4 + [2] * 5, seed=25, scale=dict(gru=2.0, lstm=3.0), lin=10.0),
    "v2049": dict(E=64, H=64, L=1, V=2049, lens=[3] * 4 + [2] * 5, seed=26, scale=dict(gru=2.0, lstm=3.0), lin=3.0),
    "tall_single": dict(E=16, H=16, L=1, V=V, lens=_lens_tall(), seed=27, scale=dict(gru=2.0, lstm=3.0), lin=6.0),
    "mid_single": dict(E=16, H=16, L=1, V=V, lens=_lens_ragged(), seed=28, scale=dict(gru=2.0, lstm=3.0), lin=6.0),
}
TRAIN_CASES = tuple(c for c in CASES if c != "h256")
ROUTE_CASES = ("e_wider", "h200", "h520")
POISON_CASES = ("e_wider", "v2047", "v2049", "tall_single")
GREEDY_CASES = ("h200", "h520", "h256", "e_wider", "v2049")
CELLS = ("gru", "lstm")


def _scaled(sd, scale, lin):
    return {k: (v * scale if k.startswith("unit.weight") else v * lin if k == "linear.weight" else v) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def problem(case, cell, bf16):
    """(params, feat (B, E), cap, lens): read-only"""
    c = CASES[case]
    params = _scaled(R.init_decoder_params(c["E"], c["H"], c["V"], c["L"], cell, seed=c["seed"]), c["scale"][cell], c["lin"])
    feat = torch.randn(len(c["lens"]), c["E"], generator=torch.Generator().manual_seed(c["seed"]))
    if bf16:
        params, feat = _bf16_params(params), _bf16(feat)
    cap, lens = captions(c["lens"], c["V"], c["seed"])
    return params, feat, cap, lens


# ====================================================================================================================
# the launch arithmetic
# ====================================================================================================================

def up8(v):
    return (v + 7) // 8 * 8


def vocab_ld(Vv):
    """st_rnn_vocab_ld (csrc/rnn.cpp)"""
    return up8(Vv) if Vv < 2048 else (Vv + 511) // 512 * 512


def dy_split(ldd, bf16):
    """the K slices of dy = dlogits W_lin in st_rnn_backward (0: one plain GEMM)"""
    bk = 64 if bf16 else 32
    return 8 if ldd % (8 * bk) == 0 and ldd >= 16 * bk else 0


def wave_steps(K, bf16):
    """skinny_mma: K is cut into steps of 4 * EPC elements and wave w of the block's four takes steps [w * spw, (w + 1) * spw) with
    spw = ceil(ns / 4).  Returns (steps of each wave, K mod (4 * EPC): the elements of a partial last step, 0 when it is full)"""
    step = 4 * (8 if bf16 else 4)
    ns = -(-K // step)
    spw = -(-ns // 4)
    return [max(0, min(ns, (w + 1) * spw) - w * spw) for w in range(4)], K % step


def gemm_launch_tiles(nc, maxM):
    """gemm_launch (csrc/rnn_kernels.hip): (MT, row tiles of the grid)"""
    mt = 2 if (nc >= 2 or maxM >= 512) and maxM > 16 else 1
    return mt, -(-maxM // (16 * mt))


def diagonals(L, bs):
    """the forward launches of st_rnn_forward: per diagonal d = l + t the (nc, maxM, MT) gemm_launch sees"""
    T, out = len(bs), []
    for d in range(T + L - 1):
        cells = [(l, d - l) for l in range(0 if d < T else d - (T - 1), L) if l <= d]
        maxM = max(bs[t] for _, t in cells)
        out.append((len(cells), maxM, gemm_launch_tiles(len(cells), maxM)[0]))
    return out


def tn_descriptors(cell, L, in0, H, Vv):
    """the token contractions of st_rnn_backward's bf16 route in the order of `tg`: (name, M, N) with C [M][N] += A^T B"""
    GH = (3 if cell == "gru" else 4) * H
    out = [("linear.weight", Vv, H)]
    for l in range(L):
        out += [(f"unit.weight_ih_l{l}", GH, in0 if l == 0 else H), (f"unit.weight_hh_l{l}", GH, H)]
    return out


def tn_tiles(M, N):
    """gemm_tn_kernel's 128 x 128 output tiles: (row tiles, column tiles, rows of the last row tile, columns of the last column
    tile) -- a tail equal to 128 is a full tile"""
    return -(-M // 128), -(-N // 128), M - 128 * ((M - 1) // 128), N - 128 * ((N - 1) // 128)


def argmax_route(H, Vv, B, bf16):
    """vocab_argmax_launch (csrc/decode.hip): ('lds' or 'generic', rpp, ysplit)"""
    es, epc = (2, 8) if bf16 else (4, 4)
    rpp = (128 * 1024 // (H * es)) & ~15
    rpp = min(rpp, (B + 15) & ~15)
    ysplit = 1
    while (Vv + 63) // 64 * ysplit < 256 and rpp >= 32 and rpp % 32 == 0 and ysplit < 4:
        ysplit *= 2
        rpp //= 2
    lds = H <= 64 * epc and H % (8 * epc) == 0 and rpp >= 16
    return ("lds" if lds else "generic"), rpp, ysplit


def paths(case, cell, bf16):
    c = CASES[case]
    E, H, L, Vv, lens = c["E"], c["H"], c["L"], c["V"], c["lens"]
    bs = R.batch_sizes(lens)
    B, ntok = len(lens), sum(lens)
    GH = (3 if cell == "gru" else 4) * H
    ld = vocab_ld(Vv)
    split = dy_split(ld, bf16)
    return dict(
        vocab_ld=ld, pad_columns=ld - Vv, dy_split=split,
        last_slice=(ld - ld // 8, ld) if split else None,        # the vocabulary columns of the eighth K slice
        maxw=max(E, H), Np=up8(ntok), ntok=ntok,
        diagonals=diagonals(L, bs),
        # forward cell: the recurrent pair has K = H, the input pair K2 = in (layer 0: E); the fused BPTT cell K = K2 = GH
        fwd_steps=dict(recurrent=wave_steps(H, bf16), input0=wave_steps(E, bf16), input=wave_steps(H, bf16)),
        bwd_steps=dict(recurrent=wave_steps(GH, bf16), input=wave_steps(GH, bf16)),
        bwd_blocks=(-(-max(bs) // 32), -(-H // 32)),             # rnn_bwd_cell_kernel: 32 rows x 32 units per block
        last_unit_tile=H - 16 * ((H - 1) // 16),                 # units in the last 16-unit tile (16: full)
        tn=[(k, M, N) + tn_tiles(M, N) for k, M, N in tn_descriptors(cell, L, E, H, Vv)],
        tn_route=bool(bf16),
        dx0_tile="128x64" if E <= 64 else "wide",                # dispatch_kc (csrc/igemm.hip): N = in0
        argmax=argmax_route(H, Vv, B, bf16),
        fused_ce=bool(bf16) and H == 512,                        # vocab_ce_supported (csrc/vocab_ce.hip)
        pipe=pipe_eligible(E, H, L, Vv, B, bf16))


# ====================================================================================================================
# the training step cell by cell: storage replica and seeded faults
# ====================================================================================================================

# what a launch that mishandles a width, a vocabulary or a batch shape would do, applied to the float64 copy
# (test_decoder_geometry_inputs.py measures each against the bounds); the K arithmetic is the bf16 kernels' (steps of 32)
#   last_unit_tile_lost          the units from 16 * floor(H / 16) on are zero (H no multiple of 16)
#   k_tail_dropped               the recurrent and input products lose their last K mod 32 terms
#   wave_without_steps_reads_on  where the four waves do not all get a K step, the last wave's share of K (the last one that has a
#                                share) is counted twice
#   pad_columns_in_softmax       logsumexp runs over Vp columns, the pad columns with zero logits
#   split_slice_lost             dy = dlogits W_lin omits the vocabulary columns of the last of the 8 K slices
#   tn_column_tail_lost          the columns of a weight gradient from 128 * floor(N / 128) on are zero
#   rows_from_512_lost           the rows of a cell from 512 on are zero
#   wide_input_truncated         layer 0 reads only the first H of its in0 columns
FAULTS = ("last_unit_tile_lost", "k_tail_dropped", "wave_without_steps_reads_on", "pad_columns_in_softmax", "split_slice_lost",
          "tn_column_tail_lost", "rows_from_512_lost", "wide_input_truncated")
# the cases each fault is aimed at: there it must move a checked quantity beyond twice its bound
AIMED = {
    "last_unit_tile_lost": ("e_wider", "h200", "h520"),
    "k_tail_dropped": ("e_wider", "h200", "h520"),
    "wave_without_steps_reads_on": ("e_wider",),
    "pad_columns_in_softmax": ("e_wider", "v2049"),
    "split_slice_lost": ("v2047",),
    "tn_column_tail_lost": ("h200", "h520"),
    "rows_from_512_lost": ("tall_single",),
    "wide_input_truncated": ("e_wider",),
}


def _idle_waves(K):
    return wave_steps(K, True)[0].count(0) > 0


def reaches(fault, case):
    """whether the fault can touch the case at all"""
    c = CASES[case]
    E, H, Vv = c["E"], c["H"], c["V"]
    if fault == "last_unit_tile_lost":
        return H % 16 != 0
    if fault == "k_tail_dropped":
        return H % 32 != 0 or E % 32 != 0
    if fault == "wave_without_steps_reads_on":
        return _idle_waves(H) or _idle_waves(E)
    if fault == "pad_columns_in_softmax":
        return vocab_ld(Vv) != Vv
    if fault == "split_slice_lost":
        ld = vocab_ld(Vv)
        return dy_split(ld, True) == 8 and ld - ld // 8 < Vv
    if fault == "tn_column_tail_lost":
        return any(N % 128 for _, _, N in tn_descriptors("gru", c["L"], E, H, Vv))
    if fault == "rows_from_512_lost":
        return len(c["lens"]) > 512
    if fault == "wide_input_truncated":
        return E > H
    raise KeyError(fault)


def _k_weights(w, fault):
    """the weight matrix [rows][K] as a faulty K walk of skinny_mma sees it"""
    K = w.shape[1]
    if fault == "k_tail_dropped" and K % 32:
        m = torch.ones(K, dtype=w.dtype)
        m[K - K % 32:] = 0
        return w * m
    if fault == "wave_without_steps_reads_on" and _idle_waves(K):
        steps, _ = wave_steps(K, True)
        busy = [i for i, s in enumerate(steps) if s]
        lo = 32 * sum(steps[:busy[-1]])
        m = torch.ones(K, dtype=w.dtype)
        m[lo:] = 2
        return w * m
    return w


class _DropSlice(torch.autograd.Function):
    """y = x W^T + b whose d loss / d x omits the vocabulary columns from `cut` on (d W and d b are whole)"""

    @staticmethod
    def forward(ctx, x, w, b, cut):
        ctx.save_for_backward(x, w)
        ctx.cut = cut
        return x @ w.t() + b

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        return g[:, :ctx.cut] @ w[:ctx.cut], g.t() @ x, g.sum(0), None


def train_copy(params, feat, cap, lens, cell, fault=None, storage=False):
    """R.gru_train_loss, one cell (l, t) at a time.  Returns (loss, packed logits).  `storage`: every forward value that
    st_rnn_forward keeps in a bf16 buffer is rounded where it is stored -- the layer-0 rows, y after every cell, c of the LSTM (the
    weights and inputs are bf16-representable already); the backward stays float64 (the recipe of tests/_decoder_depth_cases.py)."""
    st = G._stored if storage else (lambda x: x)
    L = R.num_layers_of(params)
    H = params["unit.weight_hh_l0"].shape[1]
    Vv = params["linear.weight"].shape[0]
    bs = R.batch_sizes(lens)
    T = len(bs)
    raw = torch.cat((feat.unsqueeze(1), params["embeddings.weight"][cap]), 1)      # rnn.py:29-30
    units = torch.ones(H, dtype=feat.dtype)
    if fault == "last_unit_tile_lost" and H % 16:
        units[16 * (H // 16):] = 0
    h = [[None] * T for _ in range(L)]
    c = [[None] * T for _ in range(L)]
    for t in range(T):
        bt = bs[t]
        rows = torch.ones(bt, 1, dtype=feat.dtype)
        if fault == "rows_from_512_lost":
            rows[512:] = 0
        for l in range(L):
            x = st(raw[:bt, t]) if l == 0 else h[l - 1][t]
            w_ih, w_hh, b_ih, b_hh = R._layer_w(params, l)
            if fault == "wide_input_truncated" and l == 0 and x.shape[1] > H:
                x, w_ih = x[:, :H], w_ih[:, :H]
            w_ih, w_hh = _k_weights(w_ih, fault), _k_weights(w_hh, fault)
            hp = feat.new_zeros(bt, H) if t == 0 else h[l][t - 1][:bt]
            cp = feat.new_zeros(bt, H) if t == 0 else c[l][t - 1][:bt]
            if cell == "gru":
                h[l][t], c[l][t] = st(R.gru_cell(x, hp, w_ih, w_hh, b_ih, b_hh)) * units * rows, hp
            else:
                hn, cn = R.lstm_cell(x, hp, cp, w_ih, w_hh, b_ih, b_hh)
                h[l][t], c[l][t] = st(hn) * units * rows, st(cn) * units * rows
    top = torch.cat([h[L - 1][t] for t in range(T)], 0)
    ld = vocab_ld(Vv)
    if fault == "split_slice_lost" and dy_split(ld, True) == 8:
        logits = _DropSlice.apply(top, params["linear.weight"], params["linear.bias"], ld - ld // 8)
    else:
        logits = top @ params["linear.weight"].t() + params["linear.bias"]
    target = R.pack_rows(cap, lens)
    if fault == "pad_columns_in_softmax" and ld != Vv:
        padded = torch.cat((logits, logits.new_zeros(logits.shape[0], ld - Vv)), 1)
        return R.ce_loss(padded, target), logits
    return R.ce_loss(logits, target), logits


@functools.lru_cache(maxsize=None)
def grads(case, cell, bf16=False, fault=None, storage=False):
    """float64 (loss, packed logits, {name: gradient, 'feat': d loss / d feat}) of the copy on the case's inputs"""
    params, feat, cap, lens = problem(case, cell, bf16)
    c = CASES[case]
    po = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    fo = feat.double().clone().requires_grad_(True)
    loss, logits = train_copy(po, fo, cap, lens, cell, fault, storage)
    loss.backward()
    g = {k: p.grad.detach() for k, p in po.items()}
    g["feat"] = fo.grad.detach()
    if fault == "tn_column_tail_lost":
        for k, _, N in tn_descriptors(cell, c["L"], c["E"], c["H"], c["V"]):
            if N % 128:
                g[k] = g[k].clone()
                g[k][:, 128 * (N // 128):] = 0
    return loss.item(), logits.detach(), g


def oracle_logp(case, cell, bf16, storage=False):
    """(B, T) float64 log p(cap[b, t]) of the oracle (the storage replica with `storage`)"""
    _, _, cap, lens = problem(case, cell, bf16)
    return token_logp(grads(case, cell, bf16, None, storage)[1], cap, lens)


def storage_distance(case, cell):
    """between the float64 oracle and the same oracle with bf16 rounding at the kernels' storage points, both on the
    bf16-representable inputs of the case: what bf16 storage alone does to each gradient"""
    return distance(grads(case, cell, True, None, True)[2], grads(case, cell, True)[2])


# bf16 gradients whose storage_distance reaches a quarter of the project's bound (GRAD_L2 / GRAD_MAX of
# tests/test_gpu_decoder_bench_shape.py, ROW_L2 for the rows of dfeat): (case, cell, tensor) -> (rel_l2, rel_max) as storage_distance
# gives them on the CPU.  Their bound is 4 x this distance per norm, wherever that exceeds the project's bound; every other tensor
# keeps the project's bound.  test_decoder_geometry_inputs.py recomputes the table and fails when it is stale.
STORAGE_FLOORS = {
    ('e_wider', 'gru', 'embeddings.weight'): (3.52e-03, 3.69e-03),
    ('e_wider', 'gru', 'linear.weight'): (4.13e-03, 5.42e-03),
    ('e_wider', 'gru', 'unit.bias_hh_l0'): (2.96e-03, 2.80e-03),
    ('e_wider', 'gru', 'unit.bias_hh_l1'): (2.64e-03, 3.53e-03),
    ('e_wider', 'gru', 'unit.bias_ih_l0'): (3.05e-03, 3.50e-03),
    ('e_wider', 'gru', 'unit.bias_ih_l1'): (2.52e-03, 2.31e-03),
    ('e_wider', 'gru', 'unit.weight_hh_l0'): (4.47e-03, 4.15e-03),
    ('e_wider', 'gru', 'unit.weight_hh_l1'): (4.88e-03, 5.38e-03),
    ('e_wider', 'gru', 'unit.weight_ih_l0'): (3.08e-03, 3.66e-03),
    ('e_wider', 'gru', 'unit.weight_ih_l1'): (3.75e-03, 4.27e-03),
    ('e_wider', 'lstm', 'unit.weight_hh_l0'): (2.53e-03, 4.72e-03),
}


def project_bounds(k):
    return (ROW_L2, GRAD_MAX) if k == "feat" else (GRAD_L2, GRAD_MAX)


def bf16_bounds(case, cell, k):
    """(rel_l2, rel_max) bound of one bf16 gradient: the project's, or 4 x the recorded storage floor where that is larger"""
    pl2, pmx = project_bounds(k)
    fl2, fmx = STORAGE_FLOORS.get((case, cell, k), (0.0, 0.0))
    return max(pl2, 4 * fl2), max(pmx, 4 * fmx)


def logp_distance(got, ref):
    return _rel_l2(got, ref), _rel_max(got, ref)


# token_logp is held to the gradient bounds by the same rule: (case, cell) -> the storage replica's distance from the float64
# oracle where it reaches a quarter of them
LOGP_FLOORS = {
}


def logp_bounds(case, cell):
    fl2, fmx = LOGP_FLOORS.get((case, cell), (0.0, 0.0))
    return max(GRAD_L2, 4 * fl2), max(GRAD_MAX, 4 * fmx)


# ====================================================================================================================
# greedy decoding
# ====================================================================================================================

def greedy_walk(params, feat, cell, storage, dt=torch.float64, tokens=None):
    """R.rnn_greedy (`storage`: R.rnn_greedy_bf16_storage, rounded to bf16 where the bf16 kernels store) in `dt` arithmetic; step t
    is fed tokens[:, t - 1] from the walk's OWN state, its own arg-max without `tokens`.  Returns (logits (B, STEPS, V), arg-max
    ids (B, STEPS))."""
    rnd = R._round_bf16 if storage else (lambda x: x)
    p = {k: v.to(dt) for k, v in params.items()}
    L = R.num_layers_of(p)
    B, H = feat.shape[0], p["unit.weight_hh_l0"].shape[1]
    h = [feat.new_zeros(B, H, dtype=dt) for _ in range(L)]
    c = [feat.new_zeros(B, H, dtype=dt) for _ in range(L)]
    x, out, ids = rnd(feat.to(dt)), [], []
    with torch.no_grad():
        for t in range(STEPS):
            inp = x
            for l in range(L):
                w = R._layer_w(p, l)
                if cell == "gru":
                    h[l] = rnd(R.gru_cell(inp, h[l], *w))
                else:
                    hn, cn = R.lstm_cell(inp, h[l], c[l], *w)
                    h[l], c[l] = rnd(hn), rnd(cn)
                inp = h[l]
            lg = inp @ p["linear.weight"].t() + p["linear.bias"]
            out.append(lg)
            ids.append(lg.max(1)[1])
            x = rnd(p["embeddings.weight"][ids[-1] if tokens is None else tokens[:, t]])
    return torch.stack(out, 1), torch.stack(ids, 1)


def top_two_gap(logits):
    tv = torch.topk(logits.double(), 2, dim=-1)[0]
    return tv[..., 0] - tv[..., 1]


@functools.lru_cache(maxsize=None)
def fp32_greedy_floor(case, cell):
    """the largest |d logit| between fp32 and float64 arithmetic of R.rnn_greedy on the fp32 inputs of the case, along the float64
    walk's own tokens"""
    params, feat, _, _ = problem(case, cell, False)
    l64, ids = greedy_walk(params, feat, cell, False)
    l32, _ = greedy_walk(params, feat, cell, False, torch.float32, ids)
    return (l32.double() - l64).abs().max().item()


# cell -> 4 x the largest fp32_greedy_floor over GREEDY_CASES (test_decoder_geometry_inputs.py recomputes it): an fp32 token is
# compared with the float64 walk's arg-max where that walk's top-two logit gap exceeds it.  The same test asserts that the float64
# walk leaves at most 0.10 of the steps of every case within the gap.
FP32_GAP = {"gru": 4 * 4.39e-06, "lstm": 4 * 2.81e-06}
EXCLUDED = 0.10


@functools.lru_cache(maxsize=None)
def plain_greedy_floor(case, cell):
    """tests/_decoder_depth_cases.py's plain_greedy_floor on these inputs: (share of rows that agree over all 25 steps, worst gap at
    a divergence over max |logit|) between R.rnn_greedy_bf16_storage in fp32 and in float64 arithmetic on the bf16 inputs"""
    params, feat, _, _ = problem(case, cell, True)
    l64, i64 = greedy_walk(params, feat, cell, True)
    _, i32 = greedy_walk(params, feat, cell, True, torch.float32)
    agree, worst = 0, 0.0
    for b in range(feat.shape[0]):
        d = (i32[b] != i64[b]).nonzero()
        if len(d) == 0:
            agree += 1
            continue
        lg = l64[b, int(d[0])]
        worst = max(worst, ((lg.max() - lg[i32[b, int(d[0])]]) / lg.abs().max()).item())
    return agree / feat.shape[0], worst


# (case, cell) whose plain_greedy_floor misses AGREE or DELTA: they take the looser pair _greedy_bounds gives the project's
# sensitive LSTM stack (2^-5, 2/3).  test_decoder_geometry_inputs.py recomputes the set.
GREEDY_LOOSE = ()


def greedy_bounds(case, cell):
    """(delta, agree) of a bf16 greedy check"""
    return _greedy_bounds("lstm", 5) if (case, cell) in GREEDY_LOOSE else (DELTA, AGREE)
