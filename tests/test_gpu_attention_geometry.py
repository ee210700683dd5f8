"""The soft-attention decoders over pixel counts, widths and beam slots: every code path that attn_fwd_launch, attn_bwd_launch,
attn_beam_fwd_launch (csrc/attn_kernels.hip) and make_plan (csrc/attn.cpp) choose from a shape, at the smallest shapes that take
it, GRU and LSTM, fp32 and bf16, against the float64 oracle (oracle/restatement.py; bf16: on bf16-representable weights and
features).  The other attention files run P = 49 and three width sets only.

Cases (tests/_attention_geometry_cases.py; V = 50; tests/test_attention_geometry_inputs.py asserts the paths on the CPU):
  one_pixel         P = 1, E = H = 16, F = A = 8: alpha is identically 1, the softmax backward gives zeros
  full_wave         P = 64, F = 48, A = 40: all 64 lanes of the softmax wave live; bf16 forward G = 170 pixel groups > P (empty
                    groups), 4 idle threads; backward G = 25 with 24 idle threads; a partial trip of the score loop
  tokens_gt_pixels  P = 4, 60 tokens > B*P = 28: Np comes from the tokens, every weight-gradient contraction's pad columns reversed
  odd               E = 24, F = 40, A = 24, H = 40, P = 33, L = 3: multiples of 8 and of nothing larger, 2E != H, a length-1 caption
  wide_att          A = 1032: backward G == 1 at 1024 threads with a second trip of 8 channels, 3 (bf16) / 5 (fp32) score trips
  wide_feat         F = 4104: forward G == 1 at 1024 threads (bf16 513 chunks, one trip; fp32 1026 chunks, two trips)
  many_rows         520 captions: steps of 520 rows (256-thread workgroups with G > 1 and idle threads) and of fewer than 512

A  training step, every case: loss, alphas (live rows, exact zeros past each length, row sums), every gradient.  full_wave and
   tokens_gt_pixels also through forward() + nn.CrossEntropyLoss + the alpha term; one_pixel's attention gradients are zero;
   tokens_gt_pixels twice with another case's step in between (the workspace is reused with stale contents).
B  greedy decode with attention maps: the oracle (bf16: the storage-rounded restatement at W = 1) is teacher-forced on the GPU's
   tokens from its own state; alpha at every step, the token wherever the oracle's top-two gap exceeds GAP.
C  beam widths 2, 4, 6, 7 on 3 images: the records followed as tests/test_gpu_beam_bench_shape.py follows them (its checks A to D).
D  P = 65 and W*A floats > 64 KB of LDS raise ShowTellHipError and leave the process usable.

Bounds.  A and B: the constants of tests/test_gpu_attention_bench_shape.py, unchanged, but for five bf16 gradients of wide_att LSTM
and wide_feat GRU that bf16 storage alone moves further (STORAGE_BOUNDS: 4 x the float64 distance that storage causes; their fp32
runs pass the fp32 bounds).  GAP and C: 4 x the distance between the same restatement in fp32 and in float64 arithmetic (computed
on the CPU; C on 512 images of the case's geometry, of which the GPU searches the first 3: over 3 images alone the floor is
whatever single bf16 rounding happens to flip, 3e-7 to 1e-4).  The share of steps that GAP excludes is taken over the four cases
of a cell and dtype.

Measured on the MI355X, worst over all cases (bound):
  A fp32   loss 3.2e-7 (1e-4); alphas rel_l2 4.4e-6 (1e-4) rel_max 5.0e-6 (4e-4); gradients rel_l2 1.9e-5 (1e-4) rel_max 1.7e-5 (4e-4)
           (wide_feat LSTM encoder_att.bias); drop-in against fused route 8.6e-7 / 7.2e-7
  A bf16   loss 9.8e-4 (5e-3); alphas rel_l2 4.5e-3 (1e-2) rel_max 4.8e-3 (4e-2); gradients rel_l2 2.96e-2 (3e-2) rel_max 3.1e-2 (6e-2),
           wide_feat GRU embed.weight (and embed.bias): five token rows, and bf16 storage alone moves it by 2.83e-2 / 3.1e-2 (G.storage_distance),
           the next worst is 2.0e-2; decoder_att.weight 3.8e-2 (1e-1) / 1.7e-1 (4e-1); the five gradients of STORAGE_BOUNDS below;
           drop-in against fused route 1.4e-3 (1e-2) / 3.3e-3 (4e-2)
  A both   |row sum - 1| 1.5e-7 (2e-3); |d full_att.bias| over the sum it cancels 8.4e-8 (1e-2); one_pixel attention gradients exactly 0;
           second run on a reused workspace against the first 1.3e-7 / 2.2e-7 (1e-5)
  B        alphas fp32 4.2e-6 / 5.0e-6, bf16 2.6e-4 / 5.4e-4 (bounds as A); no token differs from the oracle's arg-max at any of the
           1800 steps, within GAP or not; excluded share fp32 0.000 | 0.002, bf16 0.038 | 0.033 (0.10)
  C        after each constant below; |sum alpha - 1| 1.2e-7 (1e-5)
Runtime: the file's 77 tests take 4.3 s on the MI355X machine, float64 oracle included; the slowest (the first, which loads the
library) 0.5 s.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import _attention_geometry_cases as G
from tests._beam_oracle import check_records
from tests.test_gpu_attention import VOCAB, _make
from tests.test_gpu_attention_bench_shape import (ACCUM_L2, ACCUM_MAX, ALPHA_L2, ALPHA_MAX, F32_L2, F32_MAX, GRAD_L2, GRAD_MAX,
                                                  LOSS_REL, ROUTE_L2, ROUTE_MAX, ROW_SUM, _check_all_grads, _check_alphas,
                                                  _check_loss, _oracle)
from tests.test_gpu_decoder_bench_shape import _check_grads, _rel_l2, _rel_max

pytestmark = pytest.mark.gpu

CELLS = ["gru", "lstm"]
DTYPES = pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
ZERO_GRAD = 1e-7        # one_pixel: |attention gradient| over the largest other gradient (the oracle's are exactly zero): 0, exactly

# C: (|d nll| beyond one fp32 spacing of the cumulative cost, max |d alpha|, worst per-row relative L2 of alpha): 4 x the floor
# (fp32 against float64 arithmetic of the same restatement along the float64 oracle's own records of 512 images, the largest
# over W = 2, 4, 6, 7; test_attention_geometry_inputs.py recomputes them).  The kernels' worst values on the MI355X after the "#".
BEAM_BOUNDS = {
    ("full_wave", "gru", "fp32"): (4 * 3.83e-07, 4 * 3.24e-07, 4 * 1.04e-06),    # below one fp32 spacing of the cost, 1.45e-07, 6.60e-07
    ("full_wave", "gru", "bf16"): (4 * 8.09e-04, 4 * 1.01e-04, 4 * 5.88e-04),    # 2.65e-04, 4.42e-05, 3.24e-04 (W = 6)
    ("full_wave", "lstm", "fp32"): (4 * 3.26e-07, 4 * 2.15e-07, 4 * 8.88e-07),   # below one spacing, 7.08e-08, 4.03e-07
    ("full_wave", "lstm", "bf16"): (4 * 2.11e-04, 4 * 3.11e-05, 4 * 2.50e-04),   # below one spacing, 4.21e-08, 2.44e-07
    ("tokens_gt_pixels", "gru", "fp32"): (4 * 3.61e-07, 4 * 6.36e-07, 4 * 1.40e-06),     # below one spacing, 3.32e-07, 6.70e-07
    ("tokens_gt_pixels", "gru", "bf16"): (4 * 1.38e-03, 4 * 4.27e-04, 4 * 7.90e-04),     # 4.68e-06, 1.21e-06, 1.53e-06
    ("tokens_gt_pixels", "lstm", "fp32"): (4 * 3.29e-07, 4 * 5.15e-07, 4 * 1.04e-06),    # below one spacing, 1.91e-07, 3.82e-07
    ("tokens_gt_pixels", "lstm", "bf16"): (4 * 2.51e-04, 4 * 1.29e-04, 4 * 2.38e-04),    # 3.03e-05, 5.68e-05, 1.19e-04 (W = 6)
}

# B: 4 x the largest |d logp| between the greedy restatement in fp32 and in float64 arithmetic over GREEDY_CASES and both cells
# (fp32: the unrounded restatement; bf16: the storage-rounded one, where one stored value rounding the other way gives the
# figure); test_attention_geometry_inputs.py recomputes it
GAP = {False: 4 * 5.28e-07, True: 4 * 1.87e-03}
EXCLUDED = 0.10         # share of the walked steps of a (cell, dtype) whose top-two gap is within GAP: 0.038 (GRU bf16)

# A, bf16 only: gradients that bf16 STORAGE alone moves past GRAD_L2 / GRAD_MAX in these cases.  The kernels' fp32 runs of the same
# cases pass F32_L2 / F32_MAX, and the distance between the float64 oracle and the same oracle with bf16 rounding at make_plan's
# storage points (G.storage_distance: mean feature, h0, c0, att1, z, x, h, c) is what the GPU shows, to two digits: with B*P = 68
# (wide_att) or 18 (wide_feat) rows a rounded att1 that moves one att1 + att2 across the LeakyReLU kink changes that row's
# d u fivefold, and d att1 / d att2 have few rows to average it out.  (rel_l2, rel_max) bound = 4 x that distance; the GPU's
# values after the "#".
STORAGE_BOUNDS = {
    ("wide_att", "lstm", "attn.encoder_att.weight"): (4 * 1.74e-02, 4 * 1.54e-01),     # 1.75e-02, 1.54e-01
    ("wide_att", "lstm", "attn.encoder_att.bias"): (4 * 2.99e-02, 4 * 1.85e-01),       # 3.02e-02, 1.85e-01
    ("wide_att", "lstm", "attn.decoder_att.bias"): (4 * 2.99e-02, 4 * 1.85e-01),       # 2.99e-02, 1.86e-01
    ("wide_feat", "gru", "attn.encoder_att.bias"): (4 * 5.10e-02, 4 * 5.51e-02),       # 5.28e-02, 5.71e-02
    ("wide_feat", "gru", "attn.decoder_att.bias"): (4 * 5.10e-02, 4 * 5.51e-02),       # 5.11e-02, 5.53e-02
}

_CACHE = {}


def _beam_bounds(case, cell, bf16):
    """((words, every token), (alpha max, alpha rel_l2)) as check_records takes them; <end> has no floor of its own here"""
    nll, a_max, a_l2 = BEAM_BOUNDS[(case, cell, "bf16" if bf16 else "fp32")]
    return (nll, nll), (a_max, a_l2)


def _tag(case, cell, bf16):
    return f"{case} {cell} {'bf16' if bf16 else 'fp32'}"


def _dtype(bf16):
    return torch.bfloat16 if bf16 else torch.float32


def _reference(case, cell, bf16, monkeypatch):
    """(loss, alphas, gradients, cancelled sum) of the float64 oracle: computed once per (case, cell, dtype), read-only"""
    key = (case, cell, bf16)
    if key not in _CACHE:
        params, feat, cap, lens = G.problem(case, cell, bf16)
        _CACHE[key] = _oracle(params, feat, cap, lens, cell, monkeypatch)
    return _CACHE[key]


def _train(case, cell, bf16, route="fused"):
    """one training step on a fresh model: (loss, alphas, {name: gradient}) on the host"""
    params, feat, cap, lens = G.problem(case, cell, bf16)
    m = _make(cell, params, _dtype(bf16)).train()
    feat, cap = feat.cuda(), cap.cuda()
    if route == "fused":
        with torch.no_grad():
            _, alphas = m(feat, cap, lens)
        loss = m.loss(feat, cap, lens, 1.0)
    else:                                                   # Attention/main_attn.py:126-133
        target = nn.utils.rnn.pack_padded_sequence(cap, lens, batch_first=True)[0]
        logits, alphas = m(feat, cap, lens)
        loss = nn.CrossEntropyLoss()(logits, target) + 1.0 * ((1. - alphas.sum(dim=1)) ** 2).mean()
    loss.backward()
    torch.cuda.synchronize()
    return loss.item(), alphas.detach().cpu(), {k: p.grad.detach().double().cpu().clone() for k, p in m.named_parameters()}


def _bounds(bf16):
    return ((LOSS_REL, ALPHA_L2, ALPHA_MAX, GRAD_L2, GRAD_MAX) if bf16 else (F32_L2, F32_L2, F32_MAX, F32_L2, F32_MAX))


def _check_step(got, ref, case, cell, tag, bf16):
    """loss, alphas and every gradient; every comparison is made (and printed) before the first failure is raised"""
    loss, alphas, grads = got
    lo, al_o, g_o, cancelled = ref
    lens = G.CASES[case]["lens"]
    b = _bounds(bf16)
    failed = []

    def attempt(fn, *args):
        try:
            fn(*args)
        except AssertionError as e:
            failed.append(e)
    attempt(_check_loss, loss, lo, tag, b[0])
    attempt(_check_alphas, alphas, al_o, lens, tag, b[1], b[2])
    att = [k for k in grads if k.startswith("attn.")] if case == "one_pixel" else []
    for k, g in grads.items():
        own = STORAGE_BOUNDS.get((case, cell, k)) if bf16 else None
        if k in att:
            continue
        if own:
            attempt(_check_grads, g, g_o[k], f"{tag} grad {k} (storage bound)", *own)
        else:
            attempt(_check_all_grads, {k: g}, g_o, cancelled, tag, b[3], b[4])
    if att:
        # P = 1: alpha is identically 1, so nothing reaches the attention network; the oracle's gradients there are exactly zero
        assert len(att) == 6 and all((g_o[k] == 0).all() for k in att) and (alphas[0, :lens[0]] == 1).all()
        scale = max(g.abs().max().item() for k, g in grads.items() if k not in att)
        worst = max(grads[k].abs().max().item() for k in att)
        print(f"MEASURE {tag} attention gradients: largest |g| {worst:.2e}, {worst / scale:.2e} of the largest other gradient {scale:.2e}")
        assert worst <= ZERO_GRAD * scale
    assert not failed, failed


# ====================================================================================================================
# A. training step
# ====================================================================================================================

@DTYPES
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("case", sorted(G.CASES))
def test_training_step_matches_fp64_oracle(case, cell, bf16, monkeypatch):
    if case == "many_rows":
        rows = G.paths(case, bf16)["rows"]
        assert any(r >= 512 for r in rows) and any(r < 512 for r in rows), rows
    _check_step(_train(case, cell, bf16), _reference(case, cell, bf16, monkeypatch), case, cell, f"A {_tag(case, cell, bf16)}", bf16)


@DTYPES
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("case", ["full_wave", "tokens_gt_pixels"])
def test_dropin_route_matches_oracle_and_fused_route(case, cell, bf16, monkeypatch):
    tag = f"A {_tag(case, cell, bf16)} drop-in"
    got = _train(case, cell, bf16, "dropin")
    _check_step(got, _reference(case, cell, bf16, monkeypatch), case, cell, tag, bf16)
    fused = _train(case, cell, bf16)[2]
    l2_bound, max_bound = (ROUTE_L2, ROUTE_MAX) if bf16 else (F32_L2, F32_MAX)
    for k, g in got[2].items():
        if k == "attn.full_att.bias":
            continue
        l2, mx = _rel_l2(g, fused[k]), _rel_max(g, fused[k])
        print(f"MEASURE {tag} vs fused route {k}: rel_l2 {l2:.2e} rel_max {mx:.2e}")
        assert l2 < l2_bound and mx < max_bound, (k, l2, mx)


@DTYPES
@pytest.mark.parametrize("cell", CELLS)
def test_reused_workspace_with_stale_contents(cell, bf16, monkeypatch):
    """tokens_gt_pixels, another case's step, tokens_gt_pixels again: the allocator hands the second run a workspace that holds
    the other step's values, and Np - B*P = 36 pad columns of the encoder_att contraction lie where token rows were.  Both runs
    agree (a contraction that reads pad columns it did not zero shows here) and both match the oracle."""
    case = "tokens_gt_pixels"
    tag = f"A {_tag(case, cell, bf16)} reuse"
    first = _train(case, cell, bf16)
    _train("full_wave", cell, bf16)
    _train("odd", cell, bf16)
    second = _train(case, cell, bf16)
    _check_step(second, _reference(case, cell, bf16, monkeypatch), case, cell, tag, bf16)
    for k, g in second[2].items():
        if k == "attn.full_att.bias":
            continue
        l2, mx = _rel_l2(g, first[2][k]), _rel_max(g, first[2][k])
        print(f"MEASURE {tag} second run vs first {k}: rel_l2 {l2:.2e} rel_max {mx:.2e}")
        assert l2 < ACCUM_L2 and mx < ACCUM_MAX, (k, l2, mx)


# ====================================================================================================================
# B. greedy decode with attention maps
# ====================================================================================================================

@DTYPES
@pytest.mark.parametrize("cell", CELLS)
def test_greedy_tokens_and_maps_follow_the_oracle(cell, bf16):
    """GREEDY_CASES in turn; the excluded share is taken over the steps of all four (B * 25 each)"""
    steps = excluded = 0
    for case in G.GREEDY_CASES:
        params, feat, _, _ = G.problem(case, cell, bf16)
        B, P = feat.shape[0], feat.shape[2]
        m = _make(cell, params, _dtype(bf16)).eval()
        ids, alphas = m.sentence_index(feat.cuda(), VOCAB, return_alphas=True)
        assert torch.equal(ids, m.sentence_index(feat.cuda(), VOCAB))
        ids, alphas = ids.view(B, G.STEPS).cpu(), alphas.double().cpu()
        assert alphas.shape == (B, G.STEPS, P)
        logp, al_o, best = G.greedy_walk(params, feat, cell, bf16, tokens=ids)
        gap = G.top_two_gap(logp)
        checked = gap > GAP[bf16]
        wrong = int((ids != best)[checked].sum())
        got, ref = alphas.reshape(-1, P), al_o.double().reshape(-1, P)
        l2, mx, rs = _rel_l2(got, ref), _rel_max(got, ref), (got.sum(1) - 1).abs().max().item()
        tag = f"B {_tag(case, cell, bf16)}"
        print(f"MEASURE {tag}: alphas rel_l2 {l2:.2e} rel_max {mx:.2e} |row sum - 1| {rs:.2e}; tokens differing from the oracle's "
              f"arg-max {int((ids != best).sum())} of {ids.numel()}, {wrong} where the gap exceeds GAP = {GAP[bf16]:.2e}; steps within GAP "
              f"{int((~checked).sum())}, smallest checked gap {gap[checked].min():.2e}")
        assert l2 < (ALPHA_L2 if bf16 else F32_L2) and mx < (ALPHA_MAX if bf16 else F32_MAX) and rs < ROW_SUM, (tag, l2, mx, rs)
        assert wrong == 0, (tag, wrong)
        steps += ids.numel(); excluded += int((~checked).sum())
    print(f"MEASURE B {cell} {'bf16' if bf16 else 'fp32'}: excluded share {excluded / steps:.3f} of {steps} steps")
    assert excluded / steps <= EXCLUDED


# ====================================================================================================================
# C. beam widths
# ====================================================================================================================

@pytest.mark.parametrize("W", G.BEAM_WIDTHS)
@DTYPES
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("case", G.BEAM_CASES)
def test_beam_records_follow_the_oracle(case, cell, bf16, W):
    from showtell_amd.beam import replay_hypotheses
    assert G.V >= W
    params, feat = G.params_of(case, cell, bf16), G.beam_features(case, bf16)[:G.BEAM_IMAGES]
    key = ("model", case, cell, bf16)
    if key not in _CACHE:
        _CACHE[key] = _make(cell, params, _dtype(bf16)).eval()
    m = _CACHE[key]
    hyps, rec = m.beam_search(feat.cuda(), beam_width=W, max_length=G.BEAM_T, return_alphas=True, return_records=True)
    B, P = feat.shape[0], feat.shape[2]
    assert rec["alpha"].shape == (G.BEAM_T, B * W, P) and rec["alpha"].dtype == np.float32
    assert [[(s, c) for s, c, _ in h] for h in hyps] == replay_hypotheses(rec["tok"], rec["cost"], rec["par"], rec["end"], 1)
    assert (rec["par"][1:] >= 0).all(), "every image fills all W slots in every iteration"
    nll, alpha = _beam_bounds(case, cell, bf16)
    check_records(rec, G.beam_oracle(cell, params, feat, W, bf16), nll, f"C {_tag(case, cell, bf16)} W={W}", alpha_bounds=alpha)


# ====================================================================================================================
# D. loud failures
# ====================================================================================================================

def test_shapes_outside_the_kernels_raise_and_leave_the_process_usable(monkeypatch):
    from oracle import restatement as R
    from showtell_amd import ShowTellHipError
    case, cell = "one_pixel", "gru"
    params, feat, cap, lens = G.problem(case, cell, False)
    m = _make(cell, params, torch.float32).train()
    wide = torch.rand(1, G.CASES[case]["F"], 65).cuda()                     # P = 65
    for call in (lambda: m.loss(wide, cap.cuda(), lens, 1.0), lambda: m(wide, cap.cuda(), lens),
                 lambda: m.sentence_index(wide, VOCAB), lambda: m.sample(wide)):
        with pytest.raises(ShowTellHipError):
            call()
    # the beam launch's LDS guard: W * A floats of att2 must fit 64 KB
    sd = R.init_decoder_params(16, 16, G.V, 1, cell, seed=1, attn=dict(F=16, A=2056))
    mb = _make(cell, sd, torch.float32).eval()
    fb = G.features(2, 16, 4, 1, False).cuda()
    assert G.beam_paths(16, 2056, 4, 8, False)["lds"] > 64 * 1024 >= G.beam_paths(16, 2056, 4, 7, False)["lds"]
    with pytest.raises(ShowTellHipError):
        mb.beam_search(fb, beam_width=8, max_length=2)
    assert len(mb.beam_search(fb, beam_width=7, max_length=2)) == 2         # one slot fewer fits
    _check_step(_train(case, cell, False), _reference(case, cell, False, monkeypatch), case, cell, "D one_pixel gru fp32 after the failures", False)
