"""The host side of label smoothing, and the proof from the float64 oracle alone that the inputs and bounds of
tests/test_gpu_label_smoothing.py can catch a fault.  Nothing here needs a GPU.

Why eps = 0.3 for the bf16 cases and 0.1 for the fp32 ones: at the seeded initial weights the logits are nearly flat, the scalar
loss moves by less than 1e-3 relative under smoothing, and only the gradients and the per-row u = logsumexp - mean see it.
Dropping the smoothing in the backward pass moves every gradient by about eps * 1.4 of its scale unweighted (less under signed
weights), against a bound of 4e-2 (bf16) / 1e-3 (fp32) of that scale: the tests below print the ratios and require at least 3."""
import ctypes as C
import math

import pytest
import torch

from tests import _label_smoothing_cases as S

ALL = sorted(S.CASES)


def _cpu_decoders():
    from showtell_amd.rnn import RNN
    from showtell_amd.rnn_attn import RNN_Attn
    from showtell_amd.rnn_attn_LSTM import RNN_Attn as RNN_Attn_LSTM
    from showtell_amd.rnn_lstm import RNN as RNN_LSTM
    return [(RNN(8, 8, 20, 1), torch.zeros(3, 8)), (RNN_LSTM(8, 8, 20, 1), torch.zeros(3, 8)),
            (RNN_Attn(8, 8, 8, 8, 20, 1), torch.zeros(3, 8, 49)), (RNN_Attn_LSTM(8, 8, 8, 8, 20, 1), torch.zeros(3, 8, 49))]


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_label_smoothing_outside_0_1_is_a_value_error_before_the_device_is_touched(which):
    """On CPU tensors: a ValueError, not the 'needs a HIP device' error that anything later would raise."""
    from showtell_amd import ShowTellHipError
    m, feat = _cpu_decoders()[which]
    cap, lens = torch.tensor([[1, 5, 6, 2], [1, 7, 2, 0], [1, 2, 0, 0]]), [4, 3, 2]
    for bad in (-0.1, 1.0, float("nan"), 1.5, float("inf"), "a lot", None):
        with pytest.raises(ValueError):
            m.loss(feat, cap, lens, label_smoothing=bad)
        with pytest.raises(ValueError):
            m.loss(feat, cap, lens, sequence_weight=torch.ones(3), label_smoothing=bad)
    # well-formed values get as far as the device check: there is no CPU route
    for ok in (0.0, 0.1, 0.999):
        with pytest.raises(ShowTellHipError):
            m.loss(feat, cap, lens, label_smoothing=ok)
    with pytest.raises(ValueError):                                  # the other argument checks still run with smoothing
        m.loss(feat, cap, lens, label_smoothing=0.1, token_weight=torch.zeros(3, 3))


def test_trainer_checks_label_smoothing_and_keeps_it():
    from showtell_amd.train import Trainer

    class Opt:
        pass
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError):
            Trainer(None, None, Opt(), label_smoothing=bad)
    assert Trainer(None, None, Opt()).label_smoothing == 0.0
    assert Trainer(None, None, Opt(), label_smoothing=0.3).label_smoothing == 0.3
    assert "unsmoothed" in Trainer.step_self_critical.__doc__


def _host_descriptors(V=777, lens=(4, 3, 2)):
    """st_rnn_params / st_packed_seq whose pointers all name one small host buffer: enough for every check a C entry point makes
    before its first launch, and nothing is read through them before that."""
    from showtell_amd import _lib
    buf = C.create_string_buffer(64)
    a = C.addressof(buf)
    p = _lib.RnnParams()
    p.cell, p.dtype, p.L, p.in0, p.H, p.V, p.E = _lib.ST_CELL_GRU, _lib.ST_BF16, 1, 512, 512, V, 512
    p.emb = p.w_lin = p.b_lin = a
    p.w_ih[0] = p.w_hh[0] = p.b_ih[0] = p.b_hh[0] = a
    T = lens[0]
    bs = (C.c_int * T)(*[sum(1 for v in lens if v > t) for t in range(T)])
    s = _lib.PackedSeq(len(lens), T, sum(lens), T, bs, a, a, a, a)
    return p, s, a, (buf, bs)


def test_the_c_entry_points_refuse_a_short_tile_sums_buffer_and_a_bad_label_smoothing():
    """Checked errors of the loss entry points' st_loss_terms; each is raised on the host before anything is launched."""
    from showtell_amd import ShowTellHipError, _lib
    lib, check = _lib.lib(), _lib.check
    p, s, a, keep = _host_descriptors()
    ntok, tiles = 9, (777 + 127) // 128
    need = lib.st_rnn_fused_loss_ls_bytes(C.byref(p), C.byref(s))
    assert need == ntok * tiles * 4
    # the existing queries return what they returned: the tile sums live in a buffer of their own
    assert lib.st_rnn_fused_loss_bytes(C.byref(p), C.byref(s)) == ntok * (2 + 2 * tiles) * 4
    wb, sb = lib.st_rnn_workspace_bytes(C.byref(p), C.byref(s)), lib.st_rnn_fused_loss_bytes(C.byref(p), C.byref(s))

    def terms(smoothing, eps, smooth_out=None, tile_sums=None, tile_sums_bytes=0):
        return C.byref(_lib.LossTerms(None, None, smoothing, eps, smooth_out, tile_sums, tile_sums_bytes))

    def fused_loss(t):
        return lib.st_rnn_fused_loss(C.byref(p), C.byref(s), a, wb, a, a, sb, t, a, None, None)

    def fused_dlogits(t):
        return lib.st_rnn_fused_dlogits(C.byref(p), C.byref(s), a, wb, a, a, a, t, a, 784, None, None)

    def cross_entropy(t):
        return lib.st_cross_entropy(a, _lib.ST_F32, a, 4, 10, 16, t, a, None, 0, 16, 1.0, None, None)
    with pytest.raises(ShowTellHipError, match="tile_sums too small"):
        check(fused_loss(terms(1, 0.1, a, a, need - 4)), "short")
    with pytest.raises(ShowTellHipError, match="null pointer"):
        check(fused_loss(terms(1, 0.1, a, None, need)), "null")
    for bad in (-0.1, 1.0, float("nan")):
        for call in (fused_loss, fused_dlogits, cross_entropy):
            with pytest.raises(ShowTellHipError, match="outside"):
                check(call(terms(1, bad, a, a, need)), "eps")
    # smoothing = 0 takes none of the smoothing arguments: each is an error, not an argument that is silently ignored
    for t in (dict(eps=0.1), dict(eps=float("nan")), dict(eps=0.0, smooth_out=a), dict(eps=0.0, tile_sums=a, tile_sums_bytes=need)):
        for call in (fused_loss, fused_dlogits, cross_entropy):
            with pytest.raises(ShowTellHipError, match="smoothing = 0 takes no label_smoothing, smooth_out or tile_sums"):
                check(call(terms(0, **t)), "smoothing = 0")


def test_st_rnn_forward_refuses_a_layer_0_width_that_is_not_the_embedding_width():
    """in0 != E: the layer-0 rows are [feature ; embeddings] gathered by the call itself, there is no other source for them."""
    from showtell_amd import ShowTellHipError, _lib
    p, s, a, keep = _host_descriptors()
    p.in0 = 256
    with pytest.raises(ShowTellHipError, match=r"in0=256 != E=512"):
        _lib.check(_lib.lib().st_rnn_forward(C.byref(p), C.byref(s), a, a, 1 << 40, None, 0, 0, a, 0, None, None, None), "in0")


# ---- the inputs and bounds have power -----------------------------------------------------------------------------------------

def test_the_cases_cover_the_tile_edges_the_kernels_have():
    V = {c: S.vocab(c) for c in ALL}
    assert V["gru777"] == 777 and V["lstm1500"] == 1500 and V["gru130"] == 130 and V["gru_fp32"] == 200
    assert 777 - 6 * S.TILE == 9 and 130 - S.TILE == 2            # last tiles with 9 and 2 valid entries: one wave, three masked
    n = {c: len(S.target_of(c)) for c in ALL}
    assert n["gru777"] == 66                                          # two 32-token tiles + 2 rows
    assert n["lstm1500"] > 128                                        # more than two 64-token blocks of the reduction
    assert 2 <= n["gru130"] <= 32 and len(set(S.inputs("gru130")[3])) >= 3      # a handful of ragged captions, one token tile
    for c in ALL:
        assert S.ldd_of(c) % 8 == 0 and 0 <= S.ldd_of(c) - V[c] < 8
        x = S.oracle_rows(c)
        assert abs(x.mean().item() - S.BIAS_OFFSET) < 0.05           # the offset made the rows' mean logit 1, not 1e-3
        sw, tw = S.weights(c)
        assert (S.packed_weights(c) > 0).any() and (S.packed_weights(c) < 0).any()
    assert {S.ldd_of(c) != V[c] for c in ALL} == {True, False}       # pad columns exist (777 -> 784) and do not (200)


@pytest.mark.parametrize("case", ALL)
def test_the_bound_on_u_separates_every_seeded_fault(case):
    """The bound is 4 x what fp32 arithmetic costs on the oracle's own rows; against it, nll returned for u is at least 10 x
    outside on EVERY row, and a mean over ldd, masked lanes counted and any one tile's sum dropped are at least 10 x outside on
    their worst row.  Without the offset on linear.bias a mean over ldd would sit inside at V = 1500: the test shows that too."""
    x, bound = S.oracle_rows(case), S.u_bound(case)
    u = S.u_of(x)
    floor = S.u_floor(case)
    print(f"MEASURE {case}: floor {floor:.3e} bound {bound:.3e}  u in [{u.min().item():.4f}, {u.max().item():.4f}]")
    assert 1e-7 < floor < 2e-6                                        # an ulp or two of an fp32 near log V, not zero by luck
    faults = S.u_faults(case)
    assert "nll for u" in faults and "tile 0 dropped" in faults
    if S.ldd_of(case) != S.vocab(case):
        assert "mean over ldd" in faults
    else:
        assert case == "gru_fp32"                                     # V = 200 = ldd: there is no padded length to divide by
    for name, uf in faults.items():
        err = (uf - u).abs()
        worst, least = err.max().item(), err.min().item()
        print(f"MEASURE {case} fault '{name}': worst row {worst:.3e} ({worst / bound:.0f} x bound), least row {least:.3e}")
        assert worst >= 10 * bound, name
        if name == "nll for u":
            assert least >= 10 * bound
    # the same faults on flat logits (offset taken back): the quiet ones are the reason for the offset
    flat = x - S.BIAS_OFFSET
    lse, s, V = torch.logsumexp(flat, 1), flat.sum(1), S.vocab(case)
    if S.ldd_of(case) != V:
        quiet = (s / V - s / S.ldd_of(case)).abs().max().item()
        print(f"MEASURE {case} without the offset: mean over ldd moves u by {quiet:.3e} ({quiet / bound:.1f} x bound)")
        if case == "lstm1500":                # 4 pad columns of 1504 and a mean logit of 1e-3: the case the offset is there for
            assert quiet < 10 * bound


@pytest.mark.parametrize("case", ALL)
def test_the_dlogits_bound_holds_for_the_honest_formula_and_not_for_the_faults(case):
    """Both roundings reproduced on the CPU (fp32 arithmetic, then the output dtype): the smoothed rows stay inside
    2^-8 (bf16) / 2^-22 (fp32) * (|d0| + |expected|) on every element; a dropped term, a missing (1 - eps) and a term leaking into
    the pad columns do not.  1/ldd for 1/V moves an element by eps * (1 - V/ldd) of 1/V: outside at V = 130 (ldd = 136) and in
    fp32, inside bf16 rounding at V = 777 and 1500 (0.27 % and 0.08 % of an element against 2^-8) -- gru130 is the case that sees it."""
    eps, V, ldd = S.eps_of(case), S.vocab(case), S.ldd_of(case)
    n = len(S.target_of(case))
    gw = S.lin_weights(n).double() * 0.75 / n
    assert set(S.lin_weights(n).tolist()) == set(S.LIN_WEIGHTS)
    d0 = S.dlogits_model(case, gw, 1.0, 0.0)
    exp = S.dlogits_expected(case, d0, gw, S.target_of(case), eps)
    bound = S.dlogits_bound(case, d0, exp)

    def worst(d):
        return ((d - exp).abs() - bound).max().item(), ((d - exp).abs() / bound.clamp(min=1e-300)).max().item()
    honest = S.dlogits_model(case, gw, 1.0 - eps, eps / V)
    over, ratio = worst(honest)
    print(f"MEASURE {case}: honest formula, worst |d - expected| / bound {ratio:.3f}")
    assert over <= 0 and (honest[:, V:] == 0).all()
    faults = {"term dropped": d0, "(1 - eps) missing": S.dlogits_model(case, gw, 1.0, eps / V)}
    if ldd != V:
        faults["term in the pad columns"] = S.dlogits_model(case, gw, 1.0 - eps, eps / V, pad=-eps / V)
    for name, d in faults.items():
        over, ratio = worst(d)
        if name == "term in the pad columns":
            assert (d[:, V:] != 0).any()                              # caught by the exact-zero assertion on the pad columns
        else:
            print(f"MEASURE {case} fault '{name}': worst |d - expected| / bound {ratio:.1f}")
            assert ratio >= 10, name
    if ldd != V:
        over, ratio = worst(S.dlogits_model(case, gw, 1.0 - eps, eps / ldd))
        print(f"MEASURE {case} fault '1/ldd for 1/V': worst |d - expected| / bound {ratio:.2f}")
        if case == "gru130" or S.dtype_name(case) == "fp32":
            assert ratio > 1.5
        else:
            assert eps * (1 - V / ldd) < 2.0 ** -8                   # below one bf16 rounding of the element itself


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("case", ALL)
def test_dropping_the_smoothing_in_the_backward_pass_is_outside_the_gradient_bound(case, weighted):
    """For every parameter (and the feature): the eps = 0 gradient differs from the smoothed oracle's by at least 3 x the
    linear-form bound; and the smoothed gradient itself is not a cancellation (at least 5 % of the scale)."""
    ref, plain = S.reference(case, weighted), S.reference(case, weighted, smoothed=False)
    tol = S.GRAD_TOL[S.dtype_name(case)]
    for k in ref["g"]:
        if k in S.ZERO_GRADS:
            assert ref["g"][k].abs().max().item() < 1e-12, k
            continue
        scale = S.grad_scale(ref, k)
        move = (plain["g"][k] - ref["g"][k]).abs().max().item()
        own = ref["g"][k].abs().max().item()
        print(f"MEASURE {case} weighted={weighted} {k}: move {move / scale:.3f} of scale = {move / (tol * scale):.1f} x bound; own {own / scale:.3f}")
        assert move >= 3 * tol * scale, k
        assert own >= 0.05 * scale, k
    print(f"MEASURE {case} weighted={weighted}: loss {ref['loss']:.6f}, unsmoothed {plain['loss']:.6f}")
    assert math.isfinite(ref["loss"])
