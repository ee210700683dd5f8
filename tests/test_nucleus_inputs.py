"""Nucleus (top-p) sampling without a GPU: the oracle of tests/_nucleus_cases.py pinned to an independent restatement of the
HuggingFace rule, the power of the inputs and of the judge that tests/test_gpu_nucleus.py uses (asserted from the float64
oracle alone, with that file's bounds), six seeded faults that the judge must catch, the argument errors, and the ABI.

`python -m tests.test_nucleus_inputs` prints the figures."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from tests import _nucleus_cases as N
from tests import test_gpu_nucleus as GN
from tests import test_gpu_sample as GS
from tests import test_sample_inputs as I
from tests._util import ROOT

K_SAMPLE_CAP = 1024                    # csrc/sample.hip: the top_k candidate list; a nucleus is not bounded by it
FAULTS = ["inclusive", "high_tie", "p_before_k", "raw_logp", "next_u", "ignored"]
NEW_SYMBOLS = ["st_sample_rows_topp", "st_rnn_sample_topp", "st_attn_sample_topp"]


def _a_case(temperature, k, top_p):
    logits, u, fin, names, n = N.a_inputs()
    z = N.scaled(logits[:, :GS.ROWS_V], I.inv_temperature(temperature))
    d, b = GN._bound(GN.A_FLOOR[(temperature, k, top_p)])
    return z, u, fin == 0, names, n, d, b


def _decoder_bounds(kind, cell, storage, shape):
    return GS.bounds(kind, cell, storage, 1.0, shape, False)[:2]


# ---- the oracle ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("temperature,k,top_p", N.A_CASES)
def test_the_oracle_is_the_huggingface_rule(temperature, k, top_p):
    """TopPLogitsWarper restated: sort ASCENDING, remove where the cumulative probability is <= 1 - top_p, keep at least one.
    (Its ascending order is ours reversed: among equal values the higher index first; top-k first, by the existing oracle of
    tests/test_gpu_sample.py.)"""
    logits = GS.rows_inputs()[0]
    rows = logits[:, :GS.ROWS_V]
    inv_t = I.inv_temperature(temperature)
    _, _, _, kept = N.nucleus(rows, inv_t, k, top_p)
    lp, _ = GS.rows_oracle(rows, inv_t, k)                   # top-k and temperature, -inf outside
    V = rows.shape[1]
    asc = torch.sort(lp.flip(1), dim=1, stable=True).indices         # ascending; equal values: the higher original index first
    cum = lp.flip(1).gather(1, asc).exp().cumsum(1)
    remove = cum <= 1 - top_p
    remove[:, -1] = False
    hf = torch.zeros_like(kept).scatter_(1, (V - 1) - asc, ~remove)
    assert torch.equal(hf, kept)
    assert kept.sum(1).min() >= 1


# ---- the inputs' power ----------------------------------------------------------------------------------------------------------

def _sizes(temperature, k, top_p):
    z, u, live, names, n, d, b = _a_case(temperature, k, top_p)
    o = N.Ordered(z[:n], k)
    return o, o.prefix(top_p), names


def test_nucleus_sizes_span_one_to_beyond_the_candidate_list_and_a_tie_of_thousands():
    sizes = torch.cat([_sizes(*c)[1] for c in N.A_CASES])
    assert sizes.min() == 1 and sizes.max() > K_SAMPLE_CAP
    o, m, names = _sizes(1.0, 0, 0.9)
    assert m.min() == 1 and m.max() == 4503 and m[names["const"]] == 4503
    o, m, names = _sizes(3.0, 0, 0.9)
    assert m.median() > K_SAMPLE_CAP and m[names["tie"]] > K_SAMPLE_CAP
    # more than 256 x 4 entries of ONE value inside a nucleus, split by index: the constant row
    o, m, names = _sizes(0.7, 0, 0.5)
    assert m[names["const"]] == 2502 > 256 * 4
    assert (_sizes(1.0, 0, 1e-6)[1] == 1).all()
    assert _sizes(1.0, 32, 0.8)[1].max() <= 32 and _sizes(1.0, 5, 0.5)[1].max() <= 5


@pytest.mark.parametrize("temperature,k,top_p", N.A_CASES)
def test_the_judged_range_is_narrow(temperature, k, top_p):
    z, u, live, names, n, d, b = _a_case(temperature, k, top_p)
    o = N.Ordered(z, k)
    m_lo, m_hi = o.prefix(top_p - d), o.prefix(top_p + d)
    width, mass = (m_hi - m_lo)[live], (o.mass(m_hi) - o.mass(m_lo))[live]
    print(f"MEASURE range {temperature} {k} {top_p}: m_hi - m_lo <= {int(width.max())}, C[m_hi] - C[m_lo] <= {float(mass.max()):.2e} (4 d = {4 * d:.2e})")
    if (temperature, k, top_p) in ((0.7, 0, 0.5), (1.0, 32, 0.8)):
        assert (width == 0).all()                            # every row decided: the judge is the exact interval rule
    assert (width <= 64).all()
    # The undecided mass: every undecided entry begins inside (top_p - d, top_p + d), so all of them but the last END inside it
    # too and weigh at most 2 d together; the last one reaches beyond by its own mass, whatever d is (the constant row's
    # entries weigh 2.0e-4 each, more than 4 d).  Held to 4 d beyond that one entry.
    last = o.p.gather(1, o.order.gather(1, (m_hi - 1)[:, None]))[:, 0][live]
    assert (mass <= 4 * d + torch.where(width > 0, last, torch.zeros_like(last))).all()


@pytest.mark.parametrize("case", N.DECODER_CASES)
def test_decoder_cases_have_wide_and_single_word_nuclei(case):
    kind, cell, storage, shape, k, top_p = case
    ids, logp, lp, u = N.decoder_walk(*case)
    m = I.checked_mask(ids)
    n, T, V = lp.shape
    sizes = N.Ordered(lp.reshape(n * T, V), k).prefix(top_p).view(n, T)[m]
    d, b = _decoder_bounds(kind, cell, storage, shape)
    j = N.judge_decoder(lp, k, top_p, ids, logp, u, d, b)
    print(f"MEASURE decoder {case}: pairs {int(m.sum())}, nucleus > 1 word {float((sizes > 1).double().mean()):.2f}, "
          f"one word {float((sizes == 1).double().mean()):.2f}, largest {int(sizes.max())}")
    assert j["ok"][m].all()                                  # the oracle passes its own judge
    # the tenth of single-word nuclei is asked of the plain decoders (part D); the attention GRU at top_p = 0.9 has 0.04
    assert (sizes > 1).double().mean() >= 1 / 3 and (sizes == 1).double().mean() >= (0.1 if kind == "plain" else 0.03)


# ---- seeded faults ------------------------------------------------------------------------------------------------------------

def _a_failures(fault):
    """rows of part A (all cases, the boundary-tie row included) that fail the judge under the fault"""
    failed = {}
    for case in N.A_CASES:
        z, u, live, names, n, d, b = _a_case(*case)
        tok, logp = N.oracle_draw(z, case[1], case[2], u, fault)
        failed[case] = int((~N.judge(z, case[1], case[2], tok, logp, u, d, b)["ok"])[live].sum())
    logits, u, fin = N.tie_inputs()
    z = N.scaled(logits[:, :GS.ROWS_V], 1.0)
    d, b = GN._bound(GN.TIE_FLOOR)
    tok, logp = N.oracle_draw(z, 0, N.TIE_P, u, fault)
    failed["tie"] = int((~N.judge(z, 0, N.TIE_P, tok, logp, u, d, b)["ok"]).sum())
    return failed


def test_the_unbroken_oracle_passes_the_judge_on_every_row():
    assert not any(_a_failures(None).values())


@pytest.mark.parametrize("fault", FAULTS)
def test_seeded_faults_fail_the_judge_on_the_rows(fault):
    failed = _a_failures(fault)
    print(f"MEASURE fault {fault}: failing rows per case {failed}")
    assert sum(failed.values()) > 0
    if fault == "high_tie":
        assert failed["tie"] > 0                             # the boundary-tie row: 2000 instead of 100 at u = 0
    if fault == "p_before_k":
        assert failed[(1.0, 32, 0.8)] > 0 or failed[(1.0, 5, 0.5)] > 0
    if fault in ("inclusive", "ignored", "raw_logp"):
        assert all(failed[c] > 0 for c in N.A_CASES if c[2] != 1e-6 and c[1] == 0)


# the decoder case each fault is seeded into: fp32 storage (the tight bounds), and the top_k = 20 case for the filter order.
# 'high_tie' has no decoder case: float64 log-probabilities of 600 words have no equal pair at a nucleus boundary (asserted).
FAULT_CASE = {f: ("plain", "gru", False, (23, 11), 0, 0.9) for f in FAULTS}
FAULT_CASE["p_before_k"] = ("plain", "gru", True, (23, 11), 20, 0.9)


@pytest.mark.parametrize("fault", FAULTS)
def test_seeded_faults_fail_the_judge_on_a_decoder_case(fault):
    case = FAULT_CASE[fault]
    kind, cell, storage, shape, k, top_p = case
    ids, logp, lp, u = N.decoder_walk(*case, fault=fault)
    m = I.checked_mask(ids)
    d, b = _decoder_bounds(kind, cell, storage, shape)
    bad = ~N.judge_decoder(lp, k, top_p, ids, logp, u, d, b)["ok"]
    print(f"MEASURE fault {fault} on {case}: {int(bad[m].sum())} of {int(m.sum())} pairs fail")
    if fault == "high_tie":
        good = N.decoder_walk(*case)
        assert torch.equal(ids, good[0]) and not bad[m].any()        # no tie to split: the fault cannot show here
    else:
        assert bad[m].any()


# ---- argument errors ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_bad_top_p_is_a_value_error_before_the_device_is_touched(which):
    from showtell_amd.rnn import RNN
    from showtell_amd.rnn_attn import RNN_Attn
    from showtell_amd.rnn_attn_LSTM import RNN_Attn as RNN_Attn_LSTM
    from showtell_amd.rnn_lstm import RNN as RNN_LSTM
    a = I.ATTN
    plain, attn = (I.E, I.H, I.V, I.L), (a["E"], a["F"], a["A"], a["H"], a["V"], a["L"])
    cls, args, feat = [(RNN, plain, torch.zeros(3, I.E)), (RNN_LSTM, plain, torch.zeros(3, I.E)),
                       (RNN_Attn, attn, torch.zeros(3, a["F"], a["P"])), (RNN_Attn_LSTM, attn, torch.zeros(3, a["F"], a["P"]))][which]
    m = cls(*args)
    for bad in (0, 0.0, -0.1, 1.5, float("nan"), "0.9"):
        with pytest.raises(ValueError, match="top_p"):
            m.sample(feat, top_p=bad)
    with pytest.raises(Exception) as e:                      # a valid top_p gets past the checks, to the error of a CPU tensor
        m.sample(feat, top_p=0.9)
    assert not isinstance(e.value, ValueError)


@pytest.mark.parametrize("bad", [0.0, 1.5, float("nan")])
def test_the_c_entry_points_refuse_a_bad_top_p_ahead_of_any_launch(bad):
    """host buffers: the checks precede every launch, so nothing is read"""
    from showtell_amd import _lib
    L = _lib.lib()
    host = np.zeros(64, dtype=np.float32)
    p = C.c_void_p(host.ctypes.data)
    prm = _lib.RnnParams()
    calls = {
        "st_sample_rows_topp": lambda: L.st_sample_rows_topp(p, 8, 1, 8, p, 1, 1.0, 0, bad, 2, p, p, p, 1, 0, p, None),
        "st_rnn_sample_topp": lambda: L.st_rnn_sample_topp(C.byref(prm), p, 1, 1, p, 1.0, 0, bad, 2, p, 64, p, p, None),
        "st_attn_sample_topp": lambda: L.st_attn_sample_topp(p, p, 1, 1, 1, p, 1.0, 0, bad, 2, p, 64, p, p, None, None),
    }
    for name, call in calls.items():
        assert call() != 0, name
        assert "top_p" in L.st_last_error().decode(), name


# ---- the ABI ------------------------------------------------------------------------------------------------------------------

def test_the_new_symbols_are_declared_exported_and_bound():
    from showtell_amd import _lib
    from tests import test_abi as A
    header = A._header_text()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(raw, name) and name in _lib._SIGS and callable(getattr(_lib.lib(), name))
    sigs = A._all_sigs()
    assert A.prototype_errors(A.header_prototypes(header), sigs) == []
    assert A.symbol_set_errors(A._header_symbols(), sigs, _lib._EXPERIMENTAL) == []
    for old, new in (("st_sample_rows", "st_sample_rows_topp"), ("st_rnn_sample", "st_rnn_sample_topp"), ("st_attn_sample", "st_attn_sample_topp")):
        a, b = _lib._SIGS[old][0], _lib._SIGS[new][0]
        at = [i for i in range(len(b)) if b[:i] + b[i + 1:] == a and b[i] is C.c_float]
        assert at, (old, new)                                # the sibling's argument list with one float added


if __name__ == "__main__":
    torch.set_num_threads(8)
    for c in N.A_CASES:
        o, m, names = _sizes(*c)
        print("SIZES", c, "min %d median %d max %d const %d tie %d" % (m.min(), m.median(), m.max(), m[names["const"]], m[names["tie"]]))
