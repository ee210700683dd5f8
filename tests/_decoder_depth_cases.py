"""Cases, inputs, launch arithmetic, storage replica and seeded faults for tests/test_gpu_decoder_depth.py (GPU) and
tests/test_decoder_depth_inputs.py (CPU): the four decoders at 6 to 8 layers (ST_MAX_LAYERS = 8).  Nothing here needs a GPU.

  CASES            the case table: the smallest shapes at which depth takes each launch path of csrc/rnn.cpp / csrc/decode.hip
  problem          (params, feat, cap, lens) of one (case, cell, dtype) of the plain decoders, bf16-representable for the bf16 kernels
  attn_problem     the same for the attention decoders (F = 48, A = 40, P = 10; feat is (B, F, P))
  paths            pure-Python mirror of the launch arithmetic: the weight-gradient descriptors of st_rnn_backward in the order of
                   `gd` and their st_conv_batch groups, the cells of every wavefront diagonal, the pipelined decoder's eligibility
  train_copy       R.gru_train_loss cell by cell, with bf16 rounding where the kernels store (`storage`), the dropout masks of
                   tests/_dropout_cases.py and the seeded faults
  grads            float64 (loss, packed logits, {name: gradient, 'feat': gradient}) of the copy, cached
  storage_distance what bf16 storage alone does to each gradient; STORAGE_FLOORS is its record and bf16_bounds reads it (the replica
                   rounds the forward's stored rows; the gate cache and the gate gradients of the backward stay float64, so a floor
                   is, if anything, too low)
  oracle_logp      per-token log-probabilities of the oracle, LOGP_FLOORS / logp_bounds by the same rule
  attn_greedy_floor, plain_greedy_floor   what fp32 arithmetic alone does to the greedy restatements (ATTN_GAP; the plain one is held
                   against DELTA and AGREE by the CPU test)
  beam_*, sample_*, sched_*   inputs, oracles and fp32-against-float64 floors of the beam, sampling and scheduled-sampling checks on
                   eight_long, by the recipes of the tests those checks are borrowed from
Every table of floors is recomputed by tests/test_decoder_depth_inputs.py, which fails when a recorded figure is stale.
"""
import functools

import numpy as np
import torch

from oracle import restatement as R
from tests import _attention_geometry_cases as G
from tests import _dropout_cases as D
from tests._beam_oracle import StepOracle, beam_distance
from tests.test_gpu_decoder_bench_shape import GRAD_L2, GRAD_MAX, ROW_L2, _bf16, _bf16_params, _rel_l2, _rel_max, _row_l2

V = 50
MAX_LAYERS = 8      # ST_MAX_LAYERS (include/showtell_hip.h)
PIPE_MAXL = 5       # MAXL of csrc/decode_pipe.hip
GROUP = 12          # descriptors per st_conv_batch launch in st_rnn_backward
ATTN = dict(F=48, A=40, P=10)
ATTN_CASES = ("six", "eight_long", "eight_short")
LOGP_CASES = ("six", "eight_long")
GREEDY_CASES = ("six", "eight_long", "eight_wide")
DROPOUT_P = (0.2, 0.3, 0.5)         # (input, between layers, in front of `linear`)
DROPOUT_SEED = 0x8D0C0DE


def _lens_long():
    """B = 37, T = 10, packed batch sizes 37, 37, 35, 33, 31, 20, 17, 16, 15, 3: the drops cross a 32-row and a 16-row tile"""
    lens = [10] * 3 + [9] * 12 + [8] + [7] + [6] * 3 + [5] * 11 + [4] * 2 + [3] * 2 + [2] * 2
    assert R.batch_sizes(lens) == [37, 37, 35, 33, 31, 20, 17, 16, 15, 3]
    return lens


# `scale` (per cell) multiplies the recurrent weights (unit.weight_*), `lin` linear.weight: a freshly initialised stack attenuates,
# and at 8 layers the gradient of the lowest layers is numerically nothing.  The smallest scales at which the signal conditions of
# test_decoder_depth_inputs.py hold with room (values there) were taken: larger ones make the recurrence sensitive to bf16 storage
# (at scale 6 storage alone moves eight_long's gradients by more than their size), `lin` raises d loss / d y_top without that.
CASES = {
    #                      E     H    L  lens
    "six": dict(E=32, H=32, L=6, V=V, lens=[4, 4, 3, 2, 2], seed=11, scale=dict(gru=2.0, lstm=3.0), lin=6.0),
    "seven_narrow": dict(E=16, H=40, L=7, V=V, lens=[5, 4, 4, 2, 2], seed=12, scale=dict(gru=2.0, lstm=3.0), lin=6.0),
    "eight_long": dict(E=32, H=32, L=8, V=V, lens=_lens_long(), seed=13, scale=dict(gru=2.0, lstm=3.0), lin=6.0,
                       attn=dict(seed=dict(gru=24, lstm=27), scale=dict(gru=2.0, lstm=2.5)),      # the attention decoders' own: layer 0 must
                       # reach the logits and the greedy walk leave few steps within the gap (test_decoder_depth_inputs.py)
                       attn_beam=dict(seed=dict(gru=24, lstm=27), scale=dict(gru=2.0, lstm=3.5))),    # their beam search has no such
    # share to keep (its bounds are 4 x its own floor), and at scale 2.5 layer 0 of the LSTM reaches its logits by less than 2^-7
    "eight_short": dict(E=16, H=16, L=8, V=V, lens=[2], seed=14, scale=dict(gru=3.0, lstm=5.0), lin=6.0),
    "eight_wide": dict(E=512, H=512, L=8, V=777, lens=[3] * 20 + [2] * 13, seed=15, scale=dict(gru=3.0, lstm=5.0), lin=6.0),
}


def captions(lens, Vv, seed):
    """G.captions for a vocabulary of Vv words"""
    cap, lens = G.captions(lens, seed)
    if Vv != G.V:
        rng = np.random.RandomState(seed + 1000)
        words = (cap > 3)
        cap[words] = torch.from_numpy(rng.randint(4, Vv, size=int(words.sum())))
    return cap, lens


def _scaled(sd, scale, lin):
    return {k: (v * scale if k.startswith("unit.weight") else v * lin if k == "linear.weight" else v) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def problem(case, cell, bf16):
    """(params, feat (B, E), cap, lens) of the plain decoders: read-only"""
    c = CASES[case]
    params = _scaled(R.init_decoder_params(c["E"], c["H"], c["V"], c["L"], cell, seed=c["seed"]), c["scale"][cell], c["lin"])
    feat = torch.randn(len(c["lens"]), c["E"], generator=torch.Generator().manual_seed(c["seed"]))
    if bf16:
        params, feat = _bf16_params(params), _bf16(feat)
    cap, lens = captions(c["lens"], c["V"], c["seed"])
    return params, feat, cap, lens


@functools.lru_cache(maxsize=None)
def attn_problem(case, cell, bf16, variant="attn"):
    """(params, feat (B, F, P), cap, lens) of the attention decoders: read-only.  full_att is scaled as tests/_attention_geometry_cases.py
    scales it (a peaked alpha)"""
    c = dict(CASES[case], **CASES[case].get(variant, {}))
    if isinstance(c["seed"], dict):
        c["seed"] = c["seed"][cell]
    sd = R.init_decoder_params(c["E"], c["H"], c["V"], c["L"], cell, seed=c["seed"], attn=dict(F=ATTN["F"], A=ATTN["A"]))
    sd = _scaled(sd, c["scale"][cell], c["lin"])
    sd["attn.full_att.weight"] = sd["attn.full_att.weight"] * 8.0
    if bf16:
        sd = _bf16_params(sd)
    cap, lens = captions(c["lens"], c["V"], c["seed"])
    return sd, G.features(len(lens), ATTN["F"], ATTN["P"], c["seed"], bf16), cap, lens


# ====================================================================================================================
# the launch arithmetic
# ====================================================================================================================

def wgrad_descriptors(L, in0, H):
    """names of the weight gradients in the order st_rnn_backward (csrc/rnn.cpp) appends them to `gd`: layer by layer dW_ih (only
    where the layer's input is H wide: another width goes out as a GEMM of its own) and then dW_hh"""
    out = []
    for l in range(L):
        if (in0 if l == 0 else H) == H:
            out.append(f"unit.weight_ih_l{l}")
        out.append(f"unit.weight_hh_l{l}")
    return out


def diagonals(L, T):
    """the layers of every wavefront diagonal d = l + t, as the loops of st_rnn_forward and st_rnn_backward enumerate them"""
    return [[l for l in range(0 if d < T else d - (T - 1), L) if l <= d] for d in range(T + L - 1)]


def pipe_eligible(E, H, L, Vv, B, bf16, steps=25):
    """rnn_greedy_pipe_bytes (csrc/decode_pipe.hip) != 0"""
    if not bf16 or L < 1 or L > PIPE_MAXL or H != 512 or E != 512:
        return False
    if B < 1 or B > 256 or steps < 1 or steps > 64:
        return False
    nvw, ntile = (8 - L) * 32, (Vv + 15) // 16
    return -(-ntile // nvw) <= 8


def greedy_chain_bytes(cell, bf16, E, H, L, Vv, B):
    """make_greedy_plan (csrc/decode.hip) without the pipelined decoder's region: h[2], c[2], x, logits, keys[64 steps], gh, each at a
    256-byte boundary"""
    al = lambda v: (v + 255) // 256 * 256
    es, ng = (2 if bf16 else 4), (3 if cell == "gru" else 4)
    return 4 * al(L * B * H * es) + al(B * E * es) + al(B * ((Vv + 7) // 8 * 8) * 4) + al(B * 64 * 8) + al(L * B * ng * H * 4)


def paths(case, bf16=True):
    c = CASES[case]
    desc = wgrad_descriptors(c["L"], c["E"], c["H"])
    diag = diagonals(c["L"], c["lens"][0])
    return dict(descriptors=desc, groups=[len(desc[i:i + GROUP]) for i in range(0, len(desc), GROUP)],
                max_cells=max(len(d) for d in diag), late_start=any(d and d[0] > 0 for d in diag), diagonals=diag,
                pipe=pipe_eligible(c["E"], c["H"], c["L"], c["V"], len(c["lens"]), bf16))


# ====================================================================================================================
# the training step cell by cell: storage replica, dropout masks, seeded faults
# ====================================================================================================================

# what a wrong launch at depth would do, applied to the float64 copy (test_decoder_depth_inputs.py measures each against the bounds)
#   second_group_lost        the weight gradients of descriptors 13 and later (the second st_conv_batch group) stay zero
#   cells_capped_at_5        the sixth and later cells of a diagonal are not computed: their rows stay zero, nothing flows back
#   layer_reads_two_below    a layer l >= 6 takes y_{l-2} as its input
#   carry_of_neighbour       a layer l >= 6 receives the dh carry of layer l - 1 (and loses its own)
#   late_diagonal_from_zero  a diagonal d >= T (with L > T: most of them) counts its layers from 0: the cell of layer l runs with the
#                            weights of layer l - (d - (T - 1)) (cases with E == H only: layer 0's weights have the others' width)
#   mask_site_off_by_one     the mask of site l + 1 applied at site l, for l >= 5 (dropout runs only)
FAULTS = ("second_group_lost", "cells_capped_at_5", "layer_reads_two_below", "carry_of_neighbour", "late_diagonal_from_zero")
DROPOUT_FAULTS = ("mask_site_off_by_one",)


def reaches(fault, case):
    """whether the fault can touch the case at all"""
    c = CASES[case]
    L, T = c["L"], c["lens"][0]
    if fault == "second_group_lost":
        return len(wgrad_descriptors(L, c["E"], c["H"])) > GROUP
    if fault == "cells_capped_at_5":
        return min(L, T) > 5
    if fault == "layer_reads_two_below":
        return L >= 7
    if fault == "carry_of_neighbour":
        return L >= 7 and T >= 2
    if fault == "late_diagonal_from_zero":
        return L >= 2 and c["E"] == c["H"]
    if fault == "mask_site_off_by_one":
        return L >= 6
    raise KeyError(fault)


def site_masks(L, ntok, E, H, step=0, fault=None):
    """site -> float64 (ntok, width) multiplier of DROPOUT_P, as tests/_dropout_cases.py's _site_masks (site l < L - 1: behind layer
    l; site L - 1: in front of `linear`; D.SITE_INPUT: the layer-0 rows)"""
    p_in, p_layer, p_out = DROPOUT_P
    out = {D.SITE_INPUT: D.multiplier(DROPOUT_SEED, step, D.SITE_INPUT, ntok, E, p_in)}
    for site in range(L):
        used = site + 1 if fault == "mask_site_off_by_one" and site >= 5 else site
        out[site] = D.multiplier(DROPOUT_SEED, step, used, ntok, H, p_out if site == L - 1 else p_layer)
    return out


def train_copy(params, feat, cap, lens, cell, fault=None, storage=False, masks=None):
    """R.gru_train_loss, one cell (l, t) at a time.  Returns (loss, packed logits).
    (R._cells_storage steps all layers of one time step at once; the seeded faults act on single cells of the wavefront -- a cell
    skipped by its place on the diagonal, another layer's rows, weights or carry -- so the loop is written out here, with R's cells
    and G._stored, the rounding of tests/_attention_geometry_cases.py's replica.)
    `storage`: every forward value that st_rnn_forward keeps in a bf16 buffer is rounded where it is stored: the layer-0 rows, y
    after every cell, c of the LSTM, the dropped copies (the weights and inputs are bf16-representable already); the backward stays
    float64.  `masks`: site_masks()."""
    st = G._stored if storage else (lambda x: x)
    L = R.num_layers_of(params)
    H = params["unit.weight_hh_l0"].shape[1]
    bs = R.batch_sizes(lens)
    T, off = len(bs), np.concatenate([[0], np.cumsum(bs)])

    def drop(x, site, t):
        if masks is None:
            return x
        m = masks[site][off[t]:off[t + 1]]
        return st(D._Mask.apply(x, m, m))
    raw = torch.cat((feat.unsqueeze(1), params["embeddings.weight"][cap]), 1)      # rnn.py:29-30
    h = [[None] * T for _ in range(L)]
    c = [[None] * T for _ in range(L)]
    for t in range(T):
        bt = bs[t]
        for l in range(L):
            d = l + t
            l0 = 0 if d < T else d - (T - 1)
            if fault == "cells_capped_at_5" and l - l0 >= 5:
                h[l][t] = c[l][t] = feat.new_zeros(bt, H)
                continue
            src = l - 2 if fault == "layer_reads_two_below" and l >= 6 else l - 1
            x = drop(st(raw[:bt, t]), D.SITE_INPUT, t) if l == 0 else drop(h[src][t], src, t)
            from_zero = fault == "late_diagonal_from_zero" and d >= T and params["unit.weight_ih_l0"].shape[1] == H
            w = R._layer_w(params, l - l0 if from_zero else l)
            if t == 0:
                hp = cp = feat.new_zeros(bt, H)
            elif fault == "carry_of_neighbour":
                # the value is h_{l,t-1}; what flows back through it goes to layer l (l < 6) and to layer l + 1 (l + 1 >= 6)
                to = ([h[l][t - 1]] if l < 6 else []) + ([h[l + 1][t - 1]] if 6 <= l + 1 < L else [])
                hp = h[l][t - 1][:bt].detach() + sum(r[:bt] - r[:bt].detach() for r in to)
                cp = c[l][t - 1][:bt]
            else:
                hp, cp = h[l][t - 1][:bt], c[l][t - 1][:bt]
            if cell == "gru":
                h[l][t], c[l][t] = st(R.gru_cell(x, hp, *w)), hp
            else:
                hn, cn = R.lstm_cell(x, hp, cp, *w)
                h[l][t], c[l][t] = st(hn), st(cn)
    top = torch.cat([drop(h[L - 1][t], L - 1, t) for t in range(T)], 0)
    logits = top @ params["linear.weight"].t() + params["linear.bias"]
    return R.ce_loss(logits, R.pack_rows(cap, lens)), logits


@functools.lru_cache(maxsize=None)
def grads(case, cell, bf16=False, fault=None, storage=False, dropout=False):
    """float64 (loss, packed logits, {name: gradient, 'feat': d loss / d feat}) of the copy on the case's inputs"""
    params, feat, cap, lens = problem(case, cell, bf16)
    c = CASES[case]
    po = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    fo = feat.double().clone().requires_grad_(True)
    masks = site_masks(c["L"], sum(lens), c["E"], c["H"], 0, fault) if dropout else None
    loss, logits = train_copy(po, fo, cap, lens, cell, fault, storage, masks)
    loss.backward()
    g = {k: (torch.zeros_like(p) if p.grad is None else p.grad.detach()) for k, p in po.items()}      # None: a fault left the layer unused
    g["feat"] = fo.grad.detach()
    if fault == "second_group_lost":
        for k in wgrad_descriptors(c["L"], c["E"], c["H"])[GROUP:]:
            g[k] = torch.zeros_like(g[k])
    return loss.item(), logits.detach(), g


@functools.lru_cache(maxsize=None)
def attn_grads(case, cell, bf16=False, storage=False):
    """float64 (loss, alphas, {name: gradient}, packed logits) of G.train_copy on the attention problem of the case"""
    params, feat, cap, lens = attn_problem(case, cell, bf16)
    po = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    loss, alphas, _, logits = G.train_copy(po, feat.double(), cap, lens, cell, None, storage, return_logits=True)
    loss.backward()
    return loss.item(), alphas.detach(), {k: p.grad.detach() for k, p in po.items()}, logits.detach()


def token_logp(logits, cap, lens):
    """(B, T) log p(cap[b, t]) from packed logits, 0 past each length"""
    lp = torch.log_softmax(logits.double(), 1).gather(1, R.pack_rows(cap, lens)[:, None])[:, 0]
    out, r = torch.zeros(cap.shape, dtype=torch.float64), 0
    for t, b in enumerate(R.batch_sizes(lens)):
        out[:b, t] = lp[r:r + b]
        r += b
    return out


def distance(got, ref):
    """{tensor: (rel_l2, rel_max)}; 'feat': (worst row rel_l2, rel_max).  A tensor whose reference is all zero is left out."""
    out = {}
    for k in ref:
        if ref[k].abs().max() == 0:
            continue
        out[k] = ((_row_l2 if k == "feat" and ref[k].dim() == 2 else _rel_l2)(got[k], ref[k]), _rel_max(got[k], ref[k]))
    return out


def storage_distance(case, cell, family="plain"):
    """between the float64 oracle and the same oracle with bf16 rounding at the kernels' storage points, both on the
    bf16-representable inputs of the case: what bf16 storage alone does to each gradient"""
    if family in ("plain", "dropout"):         # "dropout": the plain decoder with the masks of DROPOUT_P on
        drop = family == "dropout"
        return distance(grads(case, cell, True, None, True, drop)[2], grads(case, cell, True, None, False, drop)[2])
    return distance(attn_grads(case, cell, True, True)[2], attn_grads(case, cell, True)[2])


# bf16 gradients whose storage_distance reaches a quarter of the project's bound (GRAD_L2 / GRAD_MAX of
# tests/test_gpu_decoder_bench_shape.py for the plain decoders, ROW_L2 for the rows of dfeat; GRAD_L2 / GRAD_MAX and DEC_ATT_* of
# tests/test_gpu_attention_bench_shape.py for the attention decoders): (family, case, cell, tensor) -> (rel_l2, rel_max) as
# storage_distance gives them on the CPU.  Their bound is 4 x this distance per norm, wherever that exceeds the project's bound;
# every other tensor keeps the project's bound.  test_decoder_depth_inputs.py recomputes the table and fails when it is stale.
STORAGE_FLOORS = {
    ('attn', 'eight_long', 'gru', 'attn.decoder_att.bias'): (3.08e-02, 3.72e-02),
    ('attn', 'eight_long', 'gru', 'attn.decoder_att.weight'): (4.08e-02, 7.22e-02),
    ('attn', 'eight_long', 'gru', 'attn.encoder_att.bias'): (3.08e-02, 3.72e-02),
    ('attn', 'eight_long', 'gru', 'attn.encoder_att.weight'): (1.92e-02, 3.37e-02),
    ('attn', 'eight_long', 'gru', 'init_h.bias'): (8.36e-03, 9.89e-03),
    ('attn', 'eight_long', 'gru', 'init_h.weight'): (8.53e-03, 1.35e-02),
    ('attn', 'eight_long', 'gru', 'unit.weight_hh_l4'): (7.68e-03, 5.17e-03),
    ('attn', 'eight_long', 'gru', 'unit.weight_hh_l5'): (7.94e-03, 7.89e-03),
    ('attn', 'eight_long', 'lstm', 'attn.decoder_att.bias'): (7.97e-03, 1.28e-02),
    ('attn', 'eight_long', 'lstm', 'attn.decoder_att.weight'): (3.56e-02, 6.44e-02),
    ('attn', 'eight_long', 'lstm', 'attn.encoder_att.bias'): (7.97e-03, 1.28e-02),
    ('attn', 'eight_long', 'lstm', 'init_h.weight'): (7.97e-03, 9.60e-03),
    ('attn', 'eight_short', 'gru', 'attn.decoder_att.bias'): (1.23e-01, 2.20e-01),
    ('attn', 'eight_short', 'gru', 'attn.decoder_att.weight'): (1.47e-01, 2.29e-01),
    ('attn', 'eight_short', 'gru', 'attn.encoder_att.bias'): (1.23e-01, 2.20e-01),
    ('attn', 'eight_short', 'gru', 'attn.encoder_att.weight'): (7.67e-02, 1.48e-01),
    ('attn', 'eight_short', 'gru', 'embed.bias'): (1.19e-02, 1.44e-02),
    ('attn', 'eight_short', 'gru', 'embed.weight'): (1.21e-02, 1.47e-02),
    ('attn', 'eight_short', 'gru', 'embeddings.weight'): (9.88e-03, 8.77e-03),
    ('attn', 'eight_short', 'gru', 'unit.bias_hh_l0'): (9.06e-03, 9.03e-03),
    ('attn', 'eight_short', 'gru', 'unit.bias_hh_l2'): (8.30e-03, 1.16e-02),
    ('attn', 'eight_short', 'gru', 'unit.bias_ih_l0'): (8.53e-03, 1.06e-02),
    ('attn', 'eight_short', 'gru', 'unit.bias_ih_l1'): (8.16e-03, 8.24e-03),
    ('attn', 'eight_short', 'gru', 'unit.bias_ih_l2'): (8.97e-03, 1.34e-02),
    ('attn', 'eight_short', 'gru', 'unit.weight_hh_l0'): (8.90e-03, 9.42e-03),
    ('attn', 'eight_short', 'gru', 'unit.weight_hh_l2'): (7.72e-03, 1.03e-02),
    ('attn', 'eight_short', 'gru', 'unit.weight_ih_l0'): (8.57e-03, 1.06e-02),
    ('attn', 'eight_short', 'gru', 'unit.weight_ih_l1'): (7.62e-03, 7.43e-03),
    ('attn', 'eight_short', 'gru', 'unit.weight_ih_l2'): (8.26e-03, 1.45e-02),
    ('attn', 'eight_short', 'gru', 'unit.weight_ih_l4'): (7.56e-03, 4.99e-03),
    ('attn', 'eight_short', 'lstm', 'embed.bias'): (2.26e-02, 2.94e-02),
    ('attn', 'eight_short', 'lstm', 'embed.weight'): (2.23e-02, 2.69e-02),
    ('attn', 'eight_short', 'lstm', 'embeddings.weight'): (1.10e-02, 7.90e-03),
    ('attn', 'eight_short', 'lstm', 'unit.bias_hh_l0'): (1.31e-02, 1.63e-02),
    ('attn', 'eight_short', 'lstm', 'unit.bias_hh_l1'): (1.17e-02, 1.61e-02),
    ('attn', 'eight_short', 'lstm', 'unit.bias_ih_l0'): (1.31e-02, 1.63e-02),
    ('attn', 'eight_short', 'lstm', 'unit.bias_ih_l1'): (1.17e-02, 1.61e-02),
    ('attn', 'eight_short', 'lstm', 'unit.weight_hh_l0'): (1.03e-02, 7.36e-03),
    ('attn', 'eight_short', 'lstm', 'unit.weight_hh_l1'): (8.42e-03, 1.12e-02),
    ('attn', 'eight_short', 'lstm', 'unit.weight_hh_l4'): (7.90e-03, 8.50e-03),
    ('attn', 'eight_short', 'lstm', 'unit.weight_ih_l0'): (1.13e-02, 1.00e-02),
    ('attn', 'eight_short', 'lstm', 'unit.weight_ih_l1'): (1.09e-02, 1.41e-02),
    ('attn', 'six', 'gru', 'attn.decoder_att.bias'): (8.78e-03, 1.06e-02),
    ('attn', 'six', 'gru', 'attn.encoder_att.bias'): (8.78e-03, 1.06e-02),
    ('dropout', 'eight_long', 'gru', 'embeddings.weight'): (7.27e-03, 8.30e-03),
    ('dropout', 'eight_long', 'gru', 'feat'): (1.78e-02, 5.50e-03),
    ('dropout', 'eight_long', 'gru', 'linear.weight'): (3.64e-03, 3.78e-03),
    ('dropout', 'eight_long', 'gru', 'unit.bias_hh_l0'): (5.70e-03, 5.07e-03),
    ('dropout', 'eight_long', 'gru', 'unit.bias_hh_l1'): (3.87e-03, 3.23e-03),
    ('dropout', 'eight_long', 'gru', 'unit.bias_hh_l2'): (3.85e-03, 2.60e-03),
    ('dropout', 'eight_long', 'gru', 'unit.bias_hh_l3'): (2.67e-03, 2.35e-03),
    ('dropout', 'eight_long', 'gru', 'unit.bias_hh_l4'): (2.59e-03, 2.60e-03),
    ('dropout', 'eight_long', 'gru', 'unit.bias_ih_l0'): (5.17e-03, 4.77e-03),
    ('dropout', 'eight_long', 'gru', 'unit.bias_ih_l1'): (3.90e-03, 3.31e-03),
    ('dropout', 'eight_long', 'gru', 'unit.bias_ih_l2'): (3.90e-03, 3.15e-03),
    ('dropout', 'eight_long', 'gru', 'unit.bias_ih_l3'): (2.65e-03, 2.71e-03),
    ('dropout', 'eight_long', 'gru', 'unit.bias_ih_l4'): (2.81e-03, 2.96e-03),
    ('dropout', 'eight_long', 'gru', 'unit.weight_hh_l0'): (7.59e-03, 6.14e-03),
    ('dropout', 'eight_long', 'gru', 'unit.weight_hh_l1'): (6.97e-03, 5.84e-03),
    ('dropout', 'eight_long', 'gru', 'unit.weight_hh_l2'): (5.79e-03, 4.08e-03),
    ('dropout', 'eight_long', 'gru', 'unit.weight_hh_l3'): (5.09e-03, 4.32e-03),
    ('dropout', 'eight_long', 'gru', 'unit.weight_hh_l4'): (4.68e-03, 3.43e-03),
    ('dropout', 'eight_long', 'gru', 'unit.weight_hh_l5'): (3.81e-03, 2.80e-03),
    ('dropout', 'eight_long', 'gru', 'unit.weight_hh_l6'): (2.99e-03, 2.38e-03),
    ('dropout', 'eight_long', 'gru', 'unit.weight_hh_l7'): (3.06e-03, 2.26e-03),
    ('dropout', 'eight_long', 'gru', 'unit.weight_ih_l0'): (6.88e-03, 4.63e-03),
    ('dropout', 'eight_long', 'gru', 'unit.weight_ih_l1'): (5.98e-03, 5.57e-03),
    ('dropout', 'eight_long', 'gru', 'unit.weight_ih_l2'): (6.10e-03, 5.79e-03),
    ('dropout', 'eight_long', 'gru', 'unit.weight_ih_l3'): (4.56e-03, 4.39e-03),
    ('dropout', 'eight_long', 'gru', 'unit.weight_ih_l4'): (4.92e-03, 2.91e-03),
    ('dropout', 'eight_long', 'gru', 'unit.weight_ih_l5'): (4.18e-03, 3.44e-03),
    ('dropout', 'eight_long', 'gru', 'unit.weight_ih_l6'): (3.51e-03, 3.31e-03),
    ('dropout', 'eight_long', 'gru', 'unit.weight_ih_l7'): (3.02e-03, 1.95e-03),
    ('dropout', 'eight_long', 'lstm', 'embeddings.weight'): (6.37e-03, 4.78e-03),
    ('dropout', 'eight_long', 'lstm', 'feat'): (1.95e-02, 6.10e-03),
    ('dropout', 'eight_long', 'lstm', 'unit.bias_hh_l0'): (7.29e-03, 5.95e-03),
    ('dropout', 'eight_long', 'lstm', 'unit.bias_hh_l1'): (3.26e-03, 3.15e-03),
    ('dropout', 'eight_long', 'lstm', 'unit.bias_ih_l0'): (7.29e-03, 5.95e-03),
    ('dropout', 'eight_long', 'lstm', 'unit.bias_ih_l1'): (3.26e-03, 3.15e-03),
    ('dropout', 'eight_long', 'lstm', 'unit.weight_hh_l0'): (8.74e-03, 8.86e-03),
    ('dropout', 'eight_long', 'lstm', 'unit.weight_hh_l1'): (7.01e-03, 5.85e-03),
    ('dropout', 'eight_long', 'lstm', 'unit.weight_hh_l2'): (4.72e-03, 3.39e-03),
    ('dropout', 'eight_long', 'lstm', 'unit.weight_hh_l3'): (3.79e-03, 5.37e-03),
    ('dropout', 'eight_long', 'lstm', 'unit.weight_hh_l5'): (2.54e-03, 2.62e-03),
    ('dropout', 'eight_long', 'lstm', 'unit.weight_ih_l0'): (6.79e-03, 5.84e-03),
    ('dropout', 'eight_long', 'lstm', 'unit.weight_ih_l1'): (5.86e-03, 5.77e-03),
    ('dropout', 'eight_long', 'lstm', 'unit.weight_ih_l2'): (5.06e-03, 4.00e-03),
    ('dropout', 'eight_long', 'lstm', 'unit.weight_ih_l3'): (3.90e-03, 3.78e-03),
    ('dropout', 'eight_long', 'lstm', 'unit.weight_ih_l4'): (2.90e-03, 2.73e-03),
    ('plain', 'eight_long', 'lstm', 'unit.weight_hh_l0'): (2.71e-03, 2.57e-03),
    ('plain', 'eight_short', 'gru', 'embeddings.weight'): (2.96e-03, 3.06e-03),
    ('plain', 'eight_short', 'gru', 'linear.weight'): (4.25e-03, 5.37e-03),
    ('plain', 'eight_short', 'gru', 'unit.bias_hh_l0'): (4.03e-03, 3.84e-03),
    ('plain', 'eight_short', 'gru', 'unit.bias_hh_l1'): (2.99e-03, 3.30e-03),
    ('plain', 'eight_short', 'gru', 'unit.bias_hh_l4'): (2.77e-03, 3.39e-03),
    ('plain', 'eight_short', 'gru', 'unit.bias_ih_l0'): (3.29e-03, 3.83e-03),
    ('plain', 'eight_short', 'gru', 'unit.bias_ih_l1'): (4.28e-03, 6.48e-03),
    ('plain', 'eight_short', 'gru', 'unit.weight_hh_l0'): (3.16e-03, 2.43e-03),
    ('plain', 'eight_short', 'gru', 'unit.weight_hh_l1'): (5.04e-03, 4.20e-03),
    ('plain', 'eight_short', 'gru', 'unit.weight_hh_l2'): (5.21e-03, 5.16e-03),
    ('plain', 'eight_short', 'gru', 'unit.weight_hh_l3'): (7.90e-03, 1.12e-02),
    ('plain', 'eight_short', 'gru', 'unit.weight_hh_l4'): (6.94e-03, 6.87e-03),
    ('plain', 'eight_short', 'gru', 'unit.weight_hh_l5'): (4.87e-03, 4.60e-03),
    ('plain', 'eight_short', 'gru', 'unit.weight_hh_l6'): (5.73e-03, 2.77e-03),
    ('plain', 'eight_short', 'gru', 'unit.weight_hh_l7'): (5.02e-03, 5.50e-03),
    ('plain', 'eight_short', 'gru', 'unit.weight_ih_l0'): (3.25e-03, 3.88e-03),
    ('plain', 'eight_short', 'gru', 'unit.weight_ih_l1'): (4.63e-03, 6.61e-03),
    ('plain', 'eight_short', 'gru', 'unit.weight_ih_l2'): (2.62e-03, 2.36e-03),
    ('plain', 'eight_short', 'gru', 'unit.weight_ih_l3'): (3.91e-03, 2.41e-03),
    ('plain', 'eight_short', 'gru', 'unit.weight_ih_l4'): (4.44e-03, 6.15e-03),
    ('plain', 'eight_short', 'gru', 'unit.weight_ih_l5'): (3.67e-03, 3.84e-03),
    ('plain', 'eight_short', 'gru', 'unit.weight_ih_l6'): (3.44e-03, 2.64e-03),
    ('plain', 'eight_short', 'gru', 'unit.weight_ih_l7'): (3.68e-03, 2.95e-03),
    ('plain', 'eight_short', 'lstm', 'embeddings.weight'): (5.61e-03, 6.45e-03),
    ('plain', 'eight_short', 'lstm', 'linear.weight'): (3.17e-03, 2.75e-03),
    ('plain', 'eight_short', 'lstm', 'unit.bias_hh_l0'): (5.76e-03, 5.76e-03),
    ('plain', 'eight_short', 'lstm', 'unit.bias_hh_l1'): (4.23e-03, 6.84e-03),
    ('plain', 'eight_short', 'lstm', 'unit.bias_hh_l2'): (2.90e-03, 2.77e-03),
    ('plain', 'eight_short', 'lstm', 'unit.bias_ih_l0'): (5.76e-03, 5.76e-03),
    ('plain', 'eight_short', 'lstm', 'unit.bias_ih_l1'): (4.23e-03, 6.84e-03),
    ('plain', 'eight_short', 'lstm', 'unit.bias_ih_l2'): (2.90e-03, 2.77e-03),
    ('plain', 'eight_short', 'lstm', 'unit.weight_hh_l0'): (7.55e-03, 9.48e-03),
    ('plain', 'eight_short', 'lstm', 'unit.weight_hh_l1'): (6.85e-03, 5.99e-03),
    ('plain', 'eight_short', 'lstm', 'unit.weight_hh_l2'): (5.34e-03, 7.01e-03),
    ('plain', 'eight_short', 'lstm', 'unit.weight_hh_l3'): (4.05e-03, 5.00e-03),
    ('plain', 'eight_short', 'lstm', 'unit.weight_hh_l4'): (3.80e-03, 3.00e-03),
    ('plain', 'eight_short', 'lstm', 'unit.weight_hh_l5'): (2.94e-03, 2.96e-03),
    ('plain', 'eight_short', 'lstm', 'unit.weight_hh_l6'): (2.64e-03, 2.49e-03),
    ('plain', 'eight_short', 'lstm', 'unit.weight_hh_l7'): (3.76e-03, 4.54e-03),
    ('plain', 'eight_short', 'lstm', 'unit.weight_ih_l0'): (5.74e-03, 5.72e-03),
    ('plain', 'eight_short', 'lstm', 'unit.weight_ih_l1'): (5.60e-03, 8.18e-03),
    ('plain', 'eight_short', 'lstm', 'unit.weight_ih_l2'): (5.14e-03, 5.60e-03),
    ('plain', 'eight_short', 'lstm', 'unit.weight_ih_l3'): (3.78e-03, 3.99e-03),
    ('plain', 'eight_short', 'lstm', 'unit.weight_ih_l4'): (2.89e-03, 2.79e-03),
    ('plain', 'eight_wide', 'gru', 'linear.weight'): (3.74e-03, 4.03e-03),
    ('plain', 'eight_wide', 'gru', 'unit.weight_hh_l0'): (5.53e-03, 5.60e-03),
    ('plain', 'eight_wide', 'gru', 'unit.weight_hh_l1'): (5.69e-03, 4.00e-03),
    ('plain', 'eight_wide', 'gru', 'unit.weight_hh_l2'): (5.53e-03, 3.27e-03),
    ('plain', 'eight_wide', 'gru', 'unit.weight_hh_l3'): (5.57e-03, 4.33e-03),
    ('plain', 'eight_wide', 'gru', 'unit.weight_hh_l4'): (5.41e-03, 3.92e-03),
    ('plain', 'eight_wide', 'gru', 'unit.weight_hh_l5'): (5.20e-03, 4.10e-03),
    ('plain', 'eight_wide', 'gru', 'unit.weight_hh_l6'): (4.91e-03, 6.22e-03),
    ('plain', 'eight_wide', 'gru', 'unit.weight_hh_l7'): (4.48e-03, 4.85e-03),
    ('plain', 'eight_wide', 'gru', 'unit.weight_ih_l0'): (3.09e-03, 2.15e-03),
    ('plain', 'eight_wide', 'gru', 'unit.weight_ih_l1'): (3.31e-03, 2.05e-03),
    ('plain', 'eight_wide', 'gru', 'unit.weight_ih_l2'): (3.33e-03, 2.31e-03),
    ('plain', 'eight_wide', 'gru', 'unit.weight_ih_l3'): (3.37e-03, 2.22e-03),
    ('plain', 'eight_wide', 'gru', 'unit.weight_ih_l4'): (3.62e-03, 2.05e-03),
    ('plain', 'eight_wide', 'gru', 'unit.weight_ih_l5'): (3.64e-03, 2.60e-03),
    ('plain', 'eight_wide', 'gru', 'unit.weight_ih_l6'): (3.67e-03, 2.91e-03),
    ('plain', 'eight_wide', 'gru', 'unit.weight_ih_l7'): (3.75e-03, 4.51e-03),
    ('plain', 'eight_wide', 'lstm', 'embeddings.weight'): (3.28e-03, 4.02e-03),
    ('plain', 'eight_wide', 'lstm', 'unit.bias_hh_l0'): (2.95e-03, 4.43e-03),
    ('plain', 'eight_wide', 'lstm', 'unit.bias_ih_l0'): (2.95e-03, 4.43e-03),
    ('plain', 'eight_wide', 'lstm', 'unit.weight_hh_l0'): (5.93e-03, 6.95e-03),
    ('plain', 'eight_wide', 'lstm', 'unit.weight_hh_l1'): (5.73e-03, 5.09e-03),
    ('plain', 'eight_wide', 'lstm', 'unit.weight_hh_l2'): (5.33e-03, 3.66e-03),
    ('plain', 'eight_wide', 'lstm', 'unit.weight_hh_l3'): (4.76e-03, 4.10e-03),
    ('plain', 'eight_wide', 'lstm', 'unit.weight_hh_l4'): (3.97e-03, 2.61e-03),
    ('plain', 'eight_wide', 'lstm', 'unit.weight_hh_l5'): (3.10e-03, 2.65e-03),
    ('plain', 'eight_wide', 'lstm', 'unit.weight_ih_l0'): (3.72e-03, 4.46e-03),
    ('plain', 'eight_wide', 'lstm', 'unit.weight_ih_l1'): (3.82e-03, 2.29e-03),
    ('plain', 'eight_wide', 'lstm', 'unit.weight_ih_l2'): (3.65e-03, 2.00e-03),
    ('plain', 'eight_wide', 'lstm', 'unit.weight_ih_l3'): (3.45e-03, 2.40e-03),
    ('plain', 'eight_wide', 'lstm', 'unit.weight_ih_l4'): (3.25e-03, 2.88e-03),
    ('plain', 'eight_wide', 'lstm', 'unit.weight_ih_l5'): (2.83e-03, 1.99e-03),
    ('plain', 'eight_wide', 'lstm', 'unit.weight_ih_l6'): (2.63e-03, 2.10e-03),
}


def project_bounds(family, k):
    """(rel_l2, rel_max) the project holds a bf16 gradient to at 5 layers"""
    if family in ("plain", "dropout"):
        return (ROW_L2, GRAD_MAX) if k == "feat" else (GRAD_L2, GRAD_MAX)
    from tests.test_gpu_attention_bench_shape import DEC_ATT_L2, DEC_ATT_MAX, GRAD_L2 as A_L2, GRAD_MAX as A_MAX
    return (DEC_ATT_L2, DEC_ATT_MAX) if k == "attn.decoder_att.weight" else (A_L2, A_MAX)


def bf16_bounds(family, case, cell, k):
    """(rel_l2, rel_max) bound of one bf16 gradient: the project's, or 4 x the recorded storage floor where that is larger"""
    pl2, pmx = project_bounds(family, k)
    fl2, fmx = STORAGE_FLOORS.get((family, case, cell, k), (0.0, 0.0))
    return max(pl2, 4 * fl2), max(pmx, 4 * fmx)


# ---- token_logp ------------------------------------------------------------------------------------------------------------------

def oracle_logp(family, case, cell, bf16, storage=False):
    """(B, T) float64 log p(cap[b, t]) of the oracle (the storage replica with `storage`)"""
    if family == "plain":
        _, _, cap, lens = problem(case, cell, bf16)
        return token_logp(grads(case, cell, bf16, None, storage)[1], cap, lens)
    _, _, cap, lens = attn_problem(case, cell, bf16)
    return token_logp(attn_grads(case, cell, bf16, storage)[3], cap, lens)


def logp_distance(got, ref):
    """(rel_l2, rel_max) of a (B, T) table of log-probabilities"""
    return _rel_l2(got, ref), _rel_max(got, ref)


# token_logp is held to the gradient bounds (GRAD_L2, GRAD_MAX: a per-element quantity read from bf16 rows), by the same rule:
# (family, case, cell) -> the storage replica's distance from the float64 oracle where it reaches a quarter of them
LOGP_FLOORS = {
}


def logp_bounds(family, case, cell):
    fl2, fmx = LOGP_FLOORS.get((family, case, cell), (0.0, 0.0))
    return max(GRAD_L2, 4 * fl2), max(GRAD_MAX, 4 * fmx)


# ---- greedy decoding of the attention decoders -------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def attn_greedy_floor(case, cell, bf16):
    """G.greedy_floor on the attention problem of the case: the largest |d logp| between fp32 and float64 arithmetic of the greedy
    restatement along the float64 walk's own tokens"""
    params, feat, _, _ = attn_problem(case, cell, bf16)
    lp64, _, ids = G.greedy_walk(params, feat, cell, bf16)
    lp32, _, _ = G.greedy_walk(params, feat, cell, bf16, torch.float32, ids)
    return (lp32.double() - lp64).abs().max().item()


ATTN_GREEDY_CASES = ("six", "eight_long")
# (cell, bf16) -> 4 x the largest attn_greedy_floor over ATTN_GREEDY_CASES (test_decoder_depth_inputs.py recomputes it): a token is
# compared with the oracle's arg-max where the oracle's top-two gap exceeds it.  The same test asserts that the float64 oracle's
# own walk leaves at most 0.09 of its steps within the gap (the GPU test allows 0.10, tests/test_gpu_attention_geometry.py).
ATTN_GAP = {("gru", False): 4 * 2.50e-06, ("gru", True): 4 * 2.13e-02, ("lstm", False): 4 * 1.10e-06, ("lstm", True): 4 * 5.85e-03}


# ---- greedy decoding of the plain bf16 decoders ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def plain_greedy_floor(case, cell):
    """(share of rows that agree over all 25 steps, worst gap at a divergence over max |logit|) between R.rnn_greedy_bf16_storage in
    fp32 and in float64 arithmetic on the bf16 inputs of the case: what any fp32 implementation of the bf16 decoder can reach, the
    measure tests/test_gpu_decoder_bench_shape.py's _greedy_bounds was set from"""
    params, feat, _, _ = problem(case, cell, True)
    with torch.no_grad():
        i64, l64 = R.rnn_greedy_bf16_storage({k: v.double() for k, v in params.items()}, feat.double(), cell)
        i32, _ = R.rnn_greedy_bf16_storage({k: v.float() for k, v in params.items()}, feat.float(), cell)
    agree, worst = 0, 0.0
    for b in range(feat.shape[0]):
        d = (i32[b] != i64[b]).nonzero()
        if len(d) == 0:
            agree += 1
            continue
        lg = l64[b, int(d[0])]
        worst = max(worst, ((lg.max() - lg[i32[b, int(d[0])]]) / lg.abs().max()).item())
    return agree / feat.shape[0], worst



# ---- beam search (eight_long, W = 4, max_length = 8, 3 images) ---------------------------------------------------------------------

BEAM_CASE = "eight_long"
BEAM_W, BEAM_T, BEAM_IMAGES, FLOOR_IMAGES = 4, 8, 3, 512      # the floors are measured on 512 images, the GPU searches the first 3
END_BOOST = 3.0     # added to linear.bias[<end>]: some hypotheses end within 8 words, so that harvesting and finished images occur


@functools.lru_cache(maxsize=None)
def beam_inputs(family, cell, bf16):
    """(params, features of FLOOR_IMAGES images of the case's geometry): read-only"""
    c = CASES[BEAM_CASE]
    params = dict(problem(BEAM_CASE, cell, bf16)[0] if family == "plain" else attn_problem(BEAM_CASE, cell, bf16, "attn_beam")[0])
    params["linear.bias"] = params["linear.bias"].clone()
    params["linear.bias"][2] += END_BOOST
    if family == "plain":
        feat = torch.randn(FLOOR_IMAGES, c["E"], generator=torch.Generator().manual_seed(c["seed"] + 500))
        return params, (_bf16(feat) if bf16 else feat)
    return params, G.features(FLOOR_IMAGES, ATTN["F"], ATTN["P"], c["seed"] + 500, bf16)


def beam_oracle(family, cell, params, feat, storage, dt=torch.float64):
    """the storage restatement of one decoder's beam step on one batch at the beam width of the case"""
    return StepOracle(family, cell, params, feat, BEAM_W, storage, dt)


@functools.lru_cache(maxsize=None)
def beam_floor(family, cell, bf16):
    """fp32 against float64 arithmetic of the same restatement, teacher-forced on the float64 oracle's own free-running records of
    FLOOR_IMAGES images (tests/_beam_oracle.beam_distance).  Returns dict(nll_word, nll, a_max, a_l2, harvested: share of the first
    BEAM_IMAGES images with a finished hypothesis)"""
    params, feat = beam_inputs(family, cell, bf16)
    o64 = beam_oracle(family, cell, params, feat, bf16)
    rec = o64.free_run(BEAM_T)
    return dict(beam_distance(beam_oracle(family, cell, params, feat, bf16, torch.float32), o64, rec),
                harvested=float(rec["end"][:, :BEAM_IMAGES].any((0, 2)).mean()))


# (family, cell, bf16) -> (|d nll| of words, of every token, max |d alpha|, worst per-row relative L2 of alpha) of beam_floor; the
# GPU test's bounds are 4 x these (test_decoder_depth_inputs.py recomputes them)
BEAM_FLOORS = {
    ("plain", "gru", False): (1.25e-06, 1.25e-06, 0.00e+00, 0.00e+00),
    ("plain", "gru", True): (7.98e-03, 7.98e-03, 0.00e+00, 0.00e+00),
    ("plain", "lstm", False): (7.74e-07, 7.74e-07, 0.00e+00, 0.00e+00),
    ("plain", "lstm", True): (3.40e-03, 3.40e-03, 0.00e+00, 0.00e+00),
    ("attn", "gru", False): (1.44e-06, 1.44e-06, 4.90e-07, 1.08e-06),
    ("attn", "gru", True): (5.96e-03, 5.96e-03, 7.96e-04, 1.94e-03),
    ("attn", "lstm", False): (1.08e-06, 1.26e-06, 2.76e-07, 6.52e-07),
    ("attn", "lstm", True): (9.07e-03, 9.07e-03, 5.76e-04, 1.23e-03),
}


def beam_bounds(family, cell, bf16):
    """((words, every token), (alpha max, alpha rel_l2) or None) as check_records of tests/_beam_oracle.py takes them"""
    w, a, amax, al2 = BEAM_FLOORS[(family, cell, bf16)]
    return (4 * w, 4 * a), ((4 * amax, 4 * al2) if family == "attn" else None)


# ---- sampling (eight_long, 2 samples per image, 6 steps) ----------------------------------------------------------------------------

SAMPLE_CASE = "eight_long"
SAMPLE_S, SAMPLE_T = 2, 6


SAMPLE_IMAGES = 37      # the GPU samples the first 37 of the FLOOR_IMAGES images the floors are measured on (over 37 images alone the
                        # floor is whatever single bf16 rounding happens to flip between fp32 and float64 sums, or none: 4e-7)


@functools.lru_cache(maxsize=None)
def sample_inputs(family, cell, bf16):
    """(params of the case, features of FLOOR_IMAGES images of its geometry, uniforms (FLOOR_IMAGES, S, T) as tests/test_sample_inputs.py
    draws them): read-only"""
    from tests import test_sample_inputs as I
    c = CASES[SAMPLE_CASE]
    params = (problem if family == "plain" else attn_problem)(SAMPLE_CASE, cell, bf16)[0]
    if family == "plain":
        feat = torch.randn(FLOOR_IMAGES, c["E"], generator=torch.Generator().manual_seed(c["seed"] + 700))
        feat = _bf16(feat) if bf16 else feat
    else:
        feat = G.features(FLOOR_IMAGES, ATTN["F"], ATTN["P"], c["seed"] + 700, bf16)
    return params, feat, I.uniforms(FLOOR_IMAGES, SAMPLE_S, SAMPLE_T)


@functools.lru_cache(maxsize=None)
def sample_floor(family, cell, bf16):
    """`_decoder_floor` of tests/test_gpu_sample.py on these inputs: (CDF, log-probability in nats, max |d alpha|) between the
    storage restatement in fp32 and in float64 arithmetic along the float64 restatement's own draws"""
    from tests import test_sample_inputs as I
    params, feat, u = sample_inputs(family, cell, bf16)
    u = u.view(-1, SAMPLE_T)
    ids, lp64, a64 = I.Oracle(family, cell, params, feat, SAMPLE_S, bf16).run(u, 1.0, steps=SAMPLE_T)
    _, lp32, a32 = I.Oracle(family, cell, params, feat, SAMPLE_S, bf16, torch.float32).run(u, 1.0, ids=ids, steps=SAMPLE_T)
    m = I.checked_mask(ids)
    cdf32 = torch.from_numpy(np.cumsum(lp32.exp().numpy(), axis=2, dtype=np.float32)).double()      # sequential float32 sum
    tok = ids[..., None]
    return (float((cdf32 - lp64.exp().cumsum(2)).abs()[m].max()),
            float((lp32.gather(2, tok).double() - lp64.gather(2, tok)).abs().squeeze(2)[m].max()),
            0.0 if a64 is None else float((a32.double() - a64).abs()[m].max()))


# (family, cell, bf16) -> sample_floor; the GPU test's bounds are 4 x these (test_decoder_depth_inputs.py recomputes them)
SAMPLE_FLOORS = {
    ("plain", "gru", False): (4.96e-07, 9.52e-07, 0.00e+00),
    ("plain", "gru", True): (1.06e-03, 7.43e-03, 0.00e+00),
    ("plain", "lstm", False): (4.77e-07, 6.14e-07, 0.00e+00),
    ("plain", "lstm", True): (2.30e-04, 2.86e-03, 0.00e+00),
    ("attn", "gru", False): (4.08e-07, 1.46e-06, 4.70e-07),
    ("attn", "gru", True): (1.03e-03, 5.81e-03, 3.38e-04),
    ("attn", "lstm", False): (4.25e-07, 6.89e-07, 3.44e-07),
    ("attn", "lstm", True): (3.33e-04, 2.54e-03, 8.10e-04),
}


def sample_bounds(family, cell, bf16):
    return tuple(4 * f for f in SAMPLE_FLOORS[(family, cell, bf16)])


# ---- scheduled sampling (eight_long, p = 0.5) ---------------------------------------------------------------------------------------

SCHED_CASE, SCHED_P = "eight_long", 0.5
SCHED_FLOOR_SEEDS = range(100, 108)


def sched_uniforms(seed=23):
    """(2, B, T) fp32 in [0, 1): [0] the coins, [1] the draws (tests/_scheduled_sampling_cases.py's layout)"""
    c = CASES[SCHED_CASE]
    return torch.rand(2, len(c["lens"]), c["lens"][0], generator=torch.Generator().manual_seed(seed))


def sched_roll_in(family, cell, bf16, u, ids=None, dt=torch.float64):
    """tests/_scheduled_sampling_cases.py's roll_in (without its faults) on the case's inputs, stepping its walker: ids None: the
    oracle mixes its own tokens, else it walks the given input ids.  Returns (input_ids (B, T), replaced (B, T), lp (B, T, V))."""
    from tests import _scheduled_sampling_cases as K

    params, feat, cap, lens = (problem if family == "plain" else attn_problem)(SCHED_CASE, cell, bf16)
    kind = "rnn" if family == "plain" else "attn"
    start, step = K.walker(kind, cell, params, feat, bf16, dt)
    Vn = params["linear.weight"].shape[0]
    B, T = cap.shape
    rep = torch.from_numpy(K.mix_rule(kind, lens, u[0].numpy(), SCHED_P))
    out = cap.clone() if ids is None else ids.clone()
    lps = torch.zeros(B, T, Vn, dtype=dt)
    with torch.no_grad():
        lp, state = start()
        first = 0 if kind == "rnn" else 1              # the first slot a step's logits decide
        if kind != "rnn":
            lp, state = step(out[:, 0], state)
        for j in range(first, max(lens) - 1 + first):
            lps[:, j] = lp
            if ids is None:
                out[:, j] = torch.where(rep[:, j], K._draw(lp, u[1][:, j]), out[:, j])
            if j + 1 < max(lens) - 1 + first:
                lp, state = step(out[:, j], state)
    return out, rep, lps


@functools.lru_cache(maxsize=None)
def sched_floor(family, cell, bf16):
    """`floor` of tests/_scheduled_sampling_cases.py: the CDF distance between fp32 and float64 arithmetic of the restatement,
    teacher-forced on the float64 oracle's own mixed ids, over every valid slot and the roll-ins of SCHED_FLOOR_SEEDS"""
    from tests import _scheduled_sampling_cases as K
    lens = CASES[SCHED_CASE]["lens"]
    worst = 0.0
    for seed in SCHED_FLOOR_SEEDS:
        u = sched_uniforms(seed)
        ids, _, lp64 = sched_roll_in(family, cell, bf16, u)
        _, _, lp32 = sched_roll_in(family, cell, bf16, u, ids=ids, dt=torch.float32)
        cdf32 = torch.from_numpy(np.cumsum(lp32.exp().numpy(), axis=2, dtype=np.float32)).double()
        m = torch.from_numpy(K.valid_slots("rnn" if family == "plain" else "attn", lens, ids.shape[1]))
        worst = max(worst, float((cdf32 - lp64.exp().cumsum(2)).abs()[m].max()))
    return worst


# (family, cell, bf16) -> sched_floor; the interval rule's d is 4 x it (test_decoder_depth_inputs.py recomputes the table)
SCHED_FLOORS = {
    ("plain", "gru", False): 4.77e-07,
    ("plain", "gru", True): 7.98e-04,
    ("plain", "lstm", False): 4.04e-07,
    ("plain", "lstm", True): 1.38e-04,
    ("attn", "gru", False): 4.19e-07,
    ("attn", "gru", True): 1.59e-03,
    ("attn", "lstm", False): 4.77e-07,
    ("attn", "lstm", True): 3.19e-04,
}
