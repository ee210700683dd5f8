"""The plain GRU / LSTM decoders over widths, vocabularies and batch shapes.  Every other GPU test of them has H in {16, 32, 40, 64,
128, 512} (one fp32 greedy call at 256), E <= H, and V >= 2048 only at E = H = 512, while the launch code picks its paths from
exactly those numbers: make_plan's maxw = max(in0, H), st_rnn_vocab_ld's two rounding rules and the 8 K slices of dy = dlogits W_lin
(csrc/rnn.cpp), gemm_launch's two-row-tile kernel and skinny_mma's K steps per wave (csrc/rnn_kernels.hip), the 128 x 128 output tiles
of the token contraction (csrc/gemm_tn.hip), the N <= 64 tile of the dx0 GEMM (csrc/igemm.hip), the LDS-staged and the generic
vocabulary arg-max (csrc/decode.hip).

Cases (tests/_decoder_geometry_cases.py; tests/test_decoder_geometry_inputs.py asserts their paths, their signal and the seeded
faults on the CPU):
  e_wider      E = 72, H = 24, V = 12, B = 5: in0 > H in every buffer and stride, dW_ih_0 a descriptor of its own with N = 72, K = 24
               less than one bf16 K step (three waves without one), K2 = 72 two steps and a quarter, four pad columns in Vp = 16
  h200         E = H = 200, B = 37 ragged: the last unit tile half full, uneven K steps per wave, two gemm_tn column tiles with a
               72-column tail, the generic arg-max in both dtypes
  h520         E = H = 520, B = 5, T = 3: the first width past 512; four gemm_tn column tiles and one 8-column chunk; the fused
               cross entropy and the pipelined decoder decline
  h256         E = H = 256, L = 1, B = 33, greedy only: the LDS-staged arg-max at a width of its own, the fp32 form's widest
  v2047/v2049  E = H = 64, L = 1, B = 9: Vp = 2048 by the round-to-8 rule and 2560 by the round-to-512 rule, both cut into 8 K
               slices; one pad column inside the last slice, or a last slice of nothing but padding
  tall_single  E = H = 16, L = 1, B = 520 (batch sizes 520, 513): one cell of 512 rows or more on the two-row-tile kernel, 17 row
               blocks in the BPTT cell, ntok = 1033 (Np = 1040)
  mid_single   E = H = 16, L = 1, B = 37 ragged: one cell of 17 to 511 rows on the one-row-tile kernel with three row tiles

A  training step: loss, token_logp, every parameter gradient and dfeat against the float64 oracle, per tensor
B  routes against each other (bf16; e_wider, h200, h520): ST_WGRAD_TN=0 and ST_BPTT_FUSED=0 under the same bounds, the default route
   twice to the bit (but for the embedding scatter and the loss, which add with atomics)
C  uninitialised memory (e_wider, v2047, v2049, tall_single): the step with every new floating-point tensor and the workspace
   filled with 0xFF bytes (NaN in fp32 and bf16) is finite and equals the plain step
D  greedy decoding (h200, h520, h256, e_wider, v2049): fp32 against the float64 walk of the GPU's own tokens, bf16 against the
   storage oracle; the fused-keys loop and the return_logits path agree
E  E = 12 and H = 20 are refused by loss, sentence_index, beam_search and sample with the multiple-of-8 message

Bounds.  fp32: FP32_REL = 2e-4 of the tensor's scale (tests/test_gpu_rnn_bptt_fused.py).  bf16 gradients: the project's GRAD_L2 /
GRAD_MAX / ROW_L2, except where bf16 storage alone, measured on the CPU between the float64 oracle and its storage replica, reaches
a quarter of them: there 4 x that distance (Y.STORAGE_FLOORS); token_logp by the same rule; the loss LOSS_REL.  Greedy: DELTA / AGREE
of tests/test_gpu_decoder_bench_shape.py (Y.greedy_bounds: no case needs the looser pair); an fp32 token is compared where the
float64 walk's top-two gap exceeds 4 x what fp32 arithmetic alone moves a logit by (Y.FP32_GAP), and at most 0.10 of the steps may
fall within it.  No bound comes from the kernels; tests/test_decoder_geometry_inputs.py recomputes every recorded floor.
"""
import ctypes as C

import pytest
import torch

from oracle import restatement as R
from tests import _decoder_geometry_cases as Y
from tests.test_gpu_decoder_bench_shape import LOSS_REL, _check_against_storage_oracle, _decoder, _rel_max, _route
from tests.test_gpu_decoder_depth import _compare
from tests.test_gpu_rnn_bptt_fused import FP32_REL

pytestmark = pytest.mark.gpu

CELLS = list(Y.CELLS)
DTYPES = pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])

# MEASURED (MI355X), worst over the cases of each check (bound):
#   A  fp32   loss 6.8e-7 (tall_single lstm), gradients max norm 7.3e-7 (h520 lstm embeddings), dfeat 1.25e-6 (h200 lstm),
#             token_logp 2.6e-7 (h200 gru)                                                                                   (2e-4)
#      bf16   loss 7.8e-4 (e_wider gru; 5e-3); gradients rel_l2 6.6e-3 (e_wider gru weight_hh_l0; its storage bound 1.8e-2), rel_max
#             6.9e-3 (e_wider lstm weight_hh_l0; 4e-2); closest to its bound: e_wider lstm weight_hh_l0, rel_l2 6.3e-3 of 1.01e-2
#             (4 x its storage floor 2.53e-3); dfeat worst row 1.45e-2 (tall_single lstm; 3e-2); token_logp rel_l2 1.2e-3, rel_max
#             1.9e-3 (e_wider gru; 1e-2, 4e-2): the storage replica's own distance
#   B  ST_WGRAD_TN=0, ST_BPTT_FUSED=0 and the default route against the oracle: the figures of A to the digits shown; the default
#      route twice, and with both variables set to 1: the same bits in every weight and bias gradient and in dfeat
#   C  the poisoned step: finite everywhere; the same bits as the plain step wherever two plain steps share them (v2047 / v2049: the
#      gradients of `linear` only, the 8 K slices of dy meet with atomics -- fp32 differed there by 3.8e-8 of the tensor's scale);
#      against the oracle the figures of A
#   D  fp32: no token of 2225 per cell differs from the float64 walk's arg-max, no step within the gap; the returned logits rel_max
#      1.0e-6 (h520 lstm; 2e-4).  bf16: every row of every case agrees with the storage oracle over all 25 steps (0.9).  The keys
#      loop and the return_logits path give the same ids in every case
#   E  twelve refusals per dtype, each with the multiple-of-8 message; mid_single trains within its bounds afterwards
# Runtime: the file's 82 tests take 4.3 s on the MI355X machine, float64 oracles included; the slowest (the first, which loads the
# library) 0.6 s.


def _tag(case, cell, bf16):
    return f"{case} {cell} {'bf16' if bf16 else 'fp32'}"


def _dtype(bf16):
    return torch.bfloat16 if bf16 else torch.float32


def _model(case, cell, bf16):
    c = Y.CASES[case]
    return _decoder(cell, Y.problem(case, cell, bf16)[0], _dtype(bf16), c["E"], c["H"], c["V"], c["L"])


def _step(m, case, cell, bf16):
    """one loss + backward: (loss, {name: gradient, 'feat': dfeat}) as float64 on the host"""
    _, feat, cap, lens = Y.problem(case, cell, bf16)
    fd = feat.cuda().requires_grad_(True)
    loss = m.loss(fd, cap.cuda(), lens)
    loss.backward()
    torch.cuda.synchronize()
    g = {k: p.grad.detach().double().cpu() for k, p in m.named_parameters()}
    g["feat"] = fd.grad.detach().double().cpu()
    return loss.item(), g


def _bounds(case, cell, bf16):
    return ((lambda k: Y.bf16_bounds(case, cell, k)) if bf16 else (lambda k: None)), (LOSS_REL if bf16 else FP32_REL)


def _clear_routes(monkeypatch):
    for k in ("ST_FUSED_CE", "ST_BPTT_FUSED", "ST_WGRAD_TN", "ST_DECODE_PIPE"):
        monkeypatch.delenv(k, raising=False)


def _same_bits_twice(k, bf16, case):
    """whether two calls of the default route give tensor `k` the same bits: the recurrence, the dx0 GEMM and the weight-gradient
    GEMMs have no atomics, nor have the bias sums of the bf16 token contraction; the embedding scatter and the fp32 route's bias
    column sums add with fp32 atomics (tests/test_gpu_rnn_bptt_fused.py, tests/test_gpu_wgrad_tn.py).  Where dy = dlogits W_lin
    runs as 8 K slices (v2047, v2049) the slices meet in memory with fp32 atomics (st_conv's split_k, csrc/igemm.hip), so only what
    does not descend from dy -- the gradients of `linear` -- keeps its bits."""
    if Y.paths(case, "gru", bf16)["dy_split"] and not k.startswith("linear"):
        return False
    return not k.startswith("embeddings") and (bf16 or "bias" not in k)


# ====================================================================================================================
# A. training step
# ====================================================================================================================

@DTYPES
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("case", Y.TRAIN_CASES)
def test_training_step_matches_fp64_oracle(case, cell, bf16, monkeypatch):
    from showtell_amd._lib import lib
    _clear_routes(monkeypatch)
    lo, _, go = Y.grads(case, cell, bf16)
    tag = f"A {_tag(case, cell, bf16)}"
    m = _model(case, cell, bf16).train()
    # the route without a logits tensor is H = 512's alone: every case here hands (n, Vp) logits and dlogits to the launch chain
    assert not lib().st_rnn_fused_loss_supported(C.byref(m._c_params()[0])) and not Y.paths(case, cell, bf16)["fused_ce"]
    assert lib().st_rnn_vocab_ld(Y.CASES[case]["V"]) == Y.paths(case, cell, bf16)["vocab_ld"]
    bounds, loss_bound = _bounds(case, cell, bf16)
    got = _step(m, case, cell, bf16)
    bad = []
    try:
        _compare(got, (lo, go), bounds, tag, loss_bound)
    except AssertionError as e:
        bad.append(e)
    _, feat, cap, lens = Y.problem(case, cell, bf16)
    lp = m.eval().token_logp(feat.cuda(), cap.cuda(), lens).double().cpu()
    ref = Y.oracle_logp(case, cell, bf16)
    assert lp.shape == ref.shape
    for b, l in enumerate(lens):
        assert (lp[b, l:] == 0).all(), (b, l)
    l2, mx = Y.logp_distance(lp, ref)
    bl2, bmx = Y.logp_bounds(case, cell) if bf16 else (FP32_REL, FP32_REL)
    print(f"MEASURE {tag} token_logp: rel_l2 {l2:.2e} rel_max {mx:.2e} (bounds {bl2:.0e}, {bmx:.0e})")
    if not (l2 < bl2 and mx < bmx):
        bad.append(("token_logp", l2, mx))
    assert not bad, (tag, bad)


# ====================================================================================================================
# B. routes against each other
# ====================================================================================================================

@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("case", Y.ROUTE_CASES)
def test_bf16_routes_agree_with_the_oracle_and_the_default_route_with_itself(case, cell, monkeypatch):
    _clear_routes(monkeypatch)
    lo, _, go = Y.grads(case, cell, True)
    tag = f"B {_tag(case, cell, True)}"
    bounds, loss_bound = _bounds(case, cell, True)
    m = _model(case, cell, True).train()
    runs = {}
    for name, env in (("default", {}), ("again", {}), ("wgrad_nt", {"ST_WGRAD_TN": "0"}), ("bptt_push", {"ST_BPTT_FUSED": "0"}),
                      ("tn_on", {"ST_WGRAD_TN": "1", "ST_BPTT_FUSED": "1"})):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            m.zero_grad()
            runs[name] = _step(m, case, cell, True)
    bad = []
    for name in ("default", "wgrad_nt", "bptt_push", "tn_on"):
        try:
            _compare(runs[name], (lo, go), bounds, f"{tag} {name}/oracle", loss_bound)
        except AssertionError as e:
            bad.append(e)
    assert not bad, (tag, bad)
    for k in runs["default"][1]:
        if _same_bits_twice(k, True, case):
            assert torch.equal(runs["default"][1][k], runs["again"][1][k]), (tag, k)
            assert torch.equal(runs["default"][1][k], runs["tn_on"][1][k]), (tag, k, "ST_WGRAD_TN=1 / ST_BPTT_FUSED=1 are the defaults")


# ====================================================================================================================
# C. uninitialised memory
# ====================================================================================================================

@DTYPES
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("case", Y.POISON_CASES)
def test_training_step_does_not_read_uninitialised_memory(case, cell, bf16, monkeypatch):
    """rnn.py allocates the workspace, the (n, Vp) logits / dlogits and dfeat with torch.empty: every pad column and pad row must
    be written before it is read, or never read.  Here torch.empty hands out floating-point tensors and uint8 buffers filled with
    0xFF bytes, which read as NaN in fp32 and bf16.  The only uint8 allocation of loss() + backward() is st_rnn_forward's workspace,
    and every region make_plan (csrc/rnn.cpp) lays out in it holds fp32 or bf16 values (x0, y, gates, cst, dyl, dx0, dgx, dgh, dhc,
    dcc, tA, tB, wT, wThh, wTih, gA, gB): no index or key lives there, so a NaN pattern cannot become an address.  Integer tensors
    (the targets, the packed-sequence tables) are left alone."""
    _clear_routes(monkeypatch)
    lo, _, go = Y.grads(case, cell, bf16)
    tag = f"C {_tag(case, cell, bf16)}"
    bounds, loss_bound = _bounds(case, cell, bf16)
    m = _model(case, cell, bf16).train()
    plain = _step(m, case, cell, bf16)
    real_empty, poisoned = torch.empty, []

    def empty(*args, **kwargs):
        t = real_empty(*args, **kwargs)
        if (t.is_floating_point() or t.dtype == torch.uint8) and t.numel() and t.is_contiguous():
            t.view(-1).view(torch.uint8).fill_(0xFF)
            poisoned.append((t.dtype, tuple(t.shape)))
        return t
    m.zero_grad()
    with monkeypatch.context() as mp:
        mp.setattr(torch, "empty", empty)
        got = _step(m, case, cell, bf16)
    n, Vp = sum(Y.CASES[case]["lens"]), Y.paths(case, cell, bf16)["vocab_ld"]
    assert (torch.uint8,) == tuple(d for d, s in poisoned if d == torch.uint8), poisoned              # the workspace, once
    assert (_dtype(bf16), (n, Vp)) in poisoned, poisoned                                              # the logits / dlogits rows
    assert (torch.float32, (len(Y.CASES[case]["lens"]), Y.CASES[case]["E"])) in poisoned, poisoned     # dfeat
    assert torch.isfinite(torch.tensor(got[0])) and all(torch.isfinite(v).all() for v in got[1].values()), \
        (tag, [k for k, v in got[1].items() if not torch.isfinite(v).all()])
    for k in got[1]:
        if _same_bits_twice(k, bf16, case):
            assert torch.equal(got[1][k], plain[1][k]), (tag, k, _rel_max(got[1][k], plain[1][k]))
    _compare(got, (lo, go), bounds, tag, loss_bound)


# ====================================================================================================================
# D. greedy decoding
# ====================================================================================================================

@DTYPES
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("case", Y.GREEDY_CASES)
def test_greedy_ids_follow_the_oracle_on_both_paths(case, cell, bf16, monkeypatch):
    _clear_routes(monkeypatch)
    params, feat, _, _ = Y.problem(case, cell, bf16)
    B = feat.shape[0]
    tag = f"D {_tag(case, cell, bf16)}"
    m = _model(case, cell, bf16).eval()
    ids = m.sentence_index(feat.cuda()).reshape(B, -1).cpu()             # keys per step, the vocabulary arg-max kernels
    assert ids.shape == (B, Y.STEPS) and _route() == 1
    ids_l, lg = m.sentence_index(feat.cuda(), return_logits=True)        # materialised logits
    assert _route() == 1
    ids_l, lg = ids_l.reshape(B, -1).cpu(), lg.double().cpu()
    assert torch.equal(ids, ids_l), (tag, int((ids != ids_l).sum()))
    assert torch.equal(lg.argmax(-1), ids), tag
    if bf16:
        with torch.no_grad():
            ids_o, lg_o = R.rnn_greedy_bf16_storage({k: v.double() for k, v in params.items()}, feat.double(), cell)
        _check_against_storage_oracle(ids, ids_o, lg_o, tag, *Y.greedy_bounds(case, cell))
        return
    l64, best = Y.greedy_walk(params, feat, cell, False, tokens=ids)
    checked = Y.top_two_gap(l64) > Y.FP32_GAP[cell]
    wrong, err = int((ids != best)[checked].sum()), _rel_max(lg, l64)
    print(f"MEASURE {tag}: tokens differing from the float64 walk's arg-max {int((ids != best).sum())} of {ids.numel()}, {wrong} where the "
          f"gap exceeds {Y.FP32_GAP[cell]:.2e}; steps within the gap {int((~checked).sum())}; logits rel_max {err:.2e} (bound {FP32_REL})")
    assert wrong == 0, (tag, wrong)
    assert int((~checked).sum()) <= Y.EXCLUDED * ids.numel(), tag
    assert err < FP32_REL, (tag, err)


# ====================================================================================================================
# E. refusals
# ====================================================================================================================

@DTYPES
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("E,H", [(12, 16), (16, 20), (12, 20)])
def test_widths_that_are_no_multiple_of_8_are_refused_by_every_entry_point(E, H, cell, bf16):
    """check_common (st_rnn_forward), st_rnn_greedy and st_rnn_step return their error ahead of any kernel launch"""
    from showtell_amd import ShowTellHipError
    params = R.init_decoder_params(E, H, Y.V, 2, cell, seed=5)
    m = _decoder(cell, params, _dtype(bf16), E, H, Y.V, 2)
    feat = torch.randn(3, E, generator=torch.Generator().manual_seed(5)).cuda()
    cap, lens = Y.captions([4, 3, 2], Y.V, 5)
    torch.cuda.synchronize()
    calls = dict(loss=lambda: m.train().loss(feat, cap.cuda(), lens), sentence_index=lambda: m.eval().sentence_index(feat),
                 beam_search=lambda: m.eval().beam_search(feat, 2, 1, 4), sample=lambda: m.eval().sample(feat, 2, 1.0, 0, 4))
    for name, call in calls.items():
        with pytest.raises(ShowTellHipError, match="must be multiples of 8") as e:
            call()
        assert f"H={H}" in str(e.value), (name, str(e.value))
    torch.cuda.synchronize()
    # the process is usable: the smallest case still trains
    got = _step(_model("mid_single", cell, bf16).train(), "mid_single", cell, bf16)
    lo, _, go = Y.grads("mid_single", cell, bf16)
    bounds, loss_bound = _bounds("mid_single", cell, bf16)
    _compare(got, (lo, go), bounds, f"E after E={E} H={H}", loss_bound)
