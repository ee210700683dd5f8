"""The plain GRU / LSTM decoders' decoding calls over widths and vocabularies: beam_search / beam_search_records / beam_search_host,
constrained beam search, sample (temperature, top_k, top_p) and scheduled_inputs.  tests/test_gpu_decoder_geometry.py took the
training step, token_logp and greedy decoding off E = H in {64, 128, 512}; these calls have host code of their own -- make_splan and
the loops of st_rnn_sample_topp / st_rnn_sched_inputs (csrc/sample.hip: x holds n * E elements beside states of L * n * H, the logits
pitch is up8(V), not training's st_rnn_vocab_ld(V)), st_rnn_step with in0 = E != H, beam._Stepper (st_embedding_rows at pitch E,
st_gather_state at H / 8 chunks per row, k = min(W, V)) -- and a stride written with H where E belongs, or a pitch taken from the
wrong rounding rule, is invisible at E = H and V < 2048.

Cases (tests/_decoding_geometry_cases.py; tests/test_decoding_geometry_inputs.py asserts their paths, their signal, the floors and
that every judge used here rejects the seeded faults, on the CPU):
  e_wider    E = 72, H = 24, L = 2, V = 12, B = 5: in0 > H; the general top-k form; four pad columns in the logits pitch
  h200       E = H = 200, B = 37: 25 chunks per gathered row, a half-full last unit tile, row counts that are no multiple of 16
  h520       E = H = 520, B = 5: the first width past 512
  v2049      E = H = 64, L = 1, V = 2049, B = 9: decoding pitch 2056 against training's 2560; the threshold top-k form up to W = 8
  v_tiny     E = H = 16, L = 1, V = 5, B = 7: at W = 8 k = V = 5 < W, 40 candidates per image, a first fringe of 5 nodes in 8 slots
  tall_beam  E = H = 16, L = 1, V = 50, B = 130: W = 4 makes 520 rows per step, S = 4 makes 520 sampled rows: the two-row-tile cell kernel

1  beam records (W in {4, 8}, max_length 8): walked by check_records of tests/_beam_oracle.py, which counts the filled slots from
   the candidates that exist (v_tiny at W = 8: a live image cannot fill 8 slots from 5 candidates); beam_search is the replay of the records; device against host selection; some hypothesis ends
2  constrained beam (e_wider, v2049; min_length 3, no_repeat_ngram_size 2, three suppressed ids): no recorded token banned for its
   parent, `hist` against the paths along `par`; an empty ban set gives the unconstrained records bit for bit
3  sample(num_samples = 2 (tall_beam: 4), max_length = 6): unfiltered, and with top_k = 3 and top_p = 0.8; the oracle walks the GPU's tokens
4  scheduled_inputs(p = 0.5) on e_wider, h200, v2049
5  st_rnn_sample and st_rnn_sched_inputs on a caller-owned workspace filled with 0xFF bytes (e_wider, v2049: pad columns in the pitch)
6  refusals: top_k > V, W * min(W, V) > 64, E = 12 / H = 20 in scheduled_inputs; the next valid call still passes

Bounds (none comes from the kernels; D.beam_bound, D.sample_bounds, D.sched_bound).  fp32: FP32_REL = 2e-4 of the scale -- of
max |logit| for a log-probability, of 1 for a cumulative probability; a top-k set is compared only where the oracle's top_k-th and
next entry lie further apart than Y.FP32_GAP, at most 0.10 of the steps may not.  bf16: 4 x the distance between the float64 oracle
and its bf16-storage replica on these inputs, measured on the CPU (D.BEAM_FLOORS, D.SAMPLE_FLOORS, D.SCHED_FLOORS); the oracle the
GPU is held to is the replica.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _decoding_geometry_cases as D
from tests.test_gpu_decoder_bench_shape import _decoder

pytestmark = pytest.mark.gpu

CELLS = list(D.CELLS)
DTYPES = pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
BEAMS = [(case, W) for case, c in D.CASES.items() for W in c["W"]]

# MEASURED (MI355X), worst over the cases of each check (bound):
#   1  beam, 20374 slots per dtype: |d nll| fp32 3.1e-6 (h200 gru W = 4; 1.0e-3), bf16 8.5e-3 (tall_beam gru; 4.2e-2 -- most cases 6e-8:
#      no stored value rounded another way than the replica's); nothing chosen above the oracle's W-th candidate, nothing missed
#      below it (at least 3.3e-5 to spare); beam_search == replay of the records; device == host selection, costs included
#   2  constrained, 1568 slots per dtype: |d nll| fp32 4.6e-7, bf16 1.5e-7; no banned token recorded, `hist` is the paths along `par`;
#      suppress_tokens=[] gives the unconstrained records bit for bit
#   3  sample, unfiltered (4220 fp32 / 4240 bf16 pairs): every draw inside the oracle's own interval (excess <= -4.7e-7 fp32, -1.7e-6
#      bf16; d 2e-4 fp32, 1.6e-3 to 7.9e-3 bf16); |d logp| fp32 2.4e-6 (h200 gru; 1.0e-3), bf16 5.6e-3 (tall_beam gru; 4.8e-2)
#      top_k = 3, top_p = 0.8 (2029 / 2026 pairs): u inside the judge's range by at least 5.2e-6 fp32, 2.3e-4 bf16; logp outside it by
#      1.1e-6 fp32, 7.1e-3 bf16 (tall_beam gru; 4.8e-2); fp32 leaves out 4 steps within Y.FP32_GAP (0.002 of them; 0.10); bf16 has 316
#      steps within its gap, judged against either top-k set, and every one passes
#   4  roll-in: `replaced` exact, 10 of 19 (e_wider), 50 of 106 (h200), 20 of 35 (v2049) valid slots; every replaced slot inside the
#      oracle's own interval (excess <= -5.0e-6 fp32, -6.2e-6 bf16)
#   5  ids, logp, replaced and drawn of the poisoned workspace equal the plain call's, bit for bit
#   6  ValueError for top_k = V + 1 (sample, sample with top_p, scheduled_inputs); ShowTellHipError "W * k <= 64" from
#      beam_search_records at W = 9 while beam_search answers as beam_search_host; "must be multiples of 8" from scheduled_inputs
# Mutation checks (each injected once, in a scratch build or by a patched method, and run over this file; not committed):
#   * st_rnn_sample_topp / st_rnn_sched_inputs hand st_embedding_rows the pitch H instead of E (in bounds, H <= E): the twelve e_wider
#     tests of 3, 4 and 5 fail and the 32 others of 3, 4 and 5 pass -- as do tests/test_gpu_sample.py and
#     tests/test_gpu_scheduled_sampling.py by construction, whose widths have E = H
#   * beam._Stepper.gather leaves every child the state of its own slot: all 52 tests of 1 and 2 fail
# Runtime: the file's 116 tests take 4.9 s on the MI355X machine, float64 oracles included; the slowest (the first, which loads the
# library) 0.5 s.

_MODELS = {}


def _tag(case, cell, bf16):
    return f"{case} {cell} {'bf16' if bf16 else 'fp32'}"


def _dtype(bf16):
    return torch.bfloat16 if bf16 else torch.float32


def _model(case, cell, bf16):
    key = (case, cell, bf16)
    if key not in _MODELS:
        c = D.CASES[case]
        _MODELS[key] = _decoder(cell, D.problem(case, cell, bf16)[0], _dtype(bf16), c["E"], c["H"], c["V"], c["L"]).eval()
    return _MODELS[key]


def _feat(case, cell, bf16):
    return D.problem(case, cell, bf16)[1].cuda()


# ====================================================================================================================
# 1. beam records
# ====================================================================================================================

@DTYPES
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("case,W", BEAMS)
def test_beam_records_follow_the_oracle(case, W, cell, bf16):
    from showtell_amd.beam import beam_search_host, beam_search_records, replay_hypotheses
    m, f, T = _model(case, cell, bf16), _feat(case, cell, bf16), D.BEAM_T
    tag = f"1 {_tag(case, cell, bf16)} W={W}"
    assert D.paths(case, W)["on_device"]
    rec = beam_search_records(m, f, W, T, D.START, D.END)
    hyps = m.beam_search(f, W, 1, T)
    assert hyps == replay_hypotheses(rec["tok"], rec["cost"], rec["par"], rec["end"], 1), tag
    host = beam_search_host(m, f, W, 1, T)
    assert len(hyps) == len(host) == D.CASES[case]["B"] and any(host)
    for d_, h_ in zip(hyps, host):
        assert [s for s, _ in d_] == [s for s, _ in h_], tag
        for (_, cd), (_, ch) in zip(d_, h_):
            assert abs(cd - ch) <= 1e-5 * max(1.0, abs(ch)), (tag, cd, ch)
    assert rec["end"].any(), "some hypothesis ends within 8 words"
    D.judge_beam(rec, case, cell, bf16, W, tag)


# ====================================================================================================================
# 2. constrained beam
# ====================================================================================================================

@DTYPES
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("case", D.CONSTRAINED_CASES)
def test_constrained_records_obey_the_ban_rule_and_an_empty_ban_set_changes_nothing(case, cell, bf16):
    from showtell_amd.beam import beam_search_records
    m, f, T = _model(case, cell, bf16), _feat(case, cell, bf16), D.BEAM_T
    mlen, g, sup = D.CONSTRAINTS
    for W in D.CASES[case]["W"]:
        tag = f"2 {_tag(case, cell, bf16)} W={W}"
        base = beam_search_records(m, f, W, T, D.START, D.END)
        empty = beam_search_records(m, f, W, T, D.START, D.END, suppress_tokens=[])
        assert set(empty) == set(base) | {"hist"}
        for key in base:
            assert base[key].dtype == empty[key].dtype and np.array_equal(base[key].view(np.uint8), empty[key].view(np.uint8)), (tag, key)
        rec = beam_search_records(m, f, W, T, D.START, D.END, min_length=mlen, no_repeat_ngram_size=g, suppress_tokens=sup)
        assert rec["hist"].shape == (D.CASES[case]["B"], W, T + 1)
        assert (rec["tok"] != base["tok"]).any(), (tag, "the constraints do not bite")
        D.judge_beam(rec, case, cell, bf16, W, tag, cons=D.CONSTRAINTS)


# ====================================================================================================================
# 3. sampling
# ====================================================================================================================

def _sample(m, case, cell, bf16, top_k, top_p):
    c = D.CASES[case]
    _, u = D.sample_rows(case, cell, bf16)
    out = m.sample(_feat(case, cell, bf16), c["S"], 1.0, top_k, D.SAMPLE_T, D.END, uniforms=u.view(c["B"], c["S"], D.SAMPLE_T).cuda(), top_p=top_p)
    ids, logp, lengths = (x.cpu() for x in out)
    assert ids.shape == logp.shape == (c["B"], c["S"], D.SAMPLE_T) and lengths.shape == (c["B"], c["S"])
    assert ids.dtype == torch.long and logp.dtype == torch.float32
    n = c["B"] * c["S"]
    return ids.view(n, -1), logp.view(n, -1), lengths.view(n)


@DTYPES
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("case", list(D.CASES))
def test_samples_follow_the_oracle(case, cell, bf16):
    m = _model(case, cell, bf16)
    tag = f"3 {_tag(case, cell, bf16)}"
    bad = []
    for top_k, top_p in ((0, 1.0), (D.TOP_K, D.TOP_P)):
        ids, logp, lengths = _sample(m, case, cell, bf16, top_k, top_p)
        try:
            fig = D.judge_sample(ids, logp, lengths, case, cell, bf16, top_k, top_p, f"{tag} top_k={top_k} top_p={top_p}")
            print(f"MEASURE {tag} top_k={top_k} top_p={top_p}: {fig}")
        except AssertionError as e:
            bad.append(e)
    assert not bad, bad


# ====================================================================================================================
# 4. roll-in
# ====================================================================================================================

@DTYPES
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("case", D.SCHED_CASES)
def test_scheduled_inputs_follow_the_oracle(case, cell, bf16):
    m = _model(case, cell, bf16)
    cap, lens, u = D.sched_problem(case)
    ids, rep = m.scheduled_inputs(_feat(case, cell, bf16), cap.cuda(), lens, D.SCHED_P, uniforms=u.cuda())
    assert ids.dtype == torch.long and rep.dtype == torch.bool
    fig = D.judge_sched(ids.cpu(), rep.cpu(), case, cell, bf16, f"4 {_tag(case, cell, bf16)}")
    print(f"MEASURE 4 {_tag(case, cell, bf16)}: {fig}")


# ====================================================================================================================
# 5. uninitialised memory
# ====================================================================================================================

def _poisoned(nbytes):
    return torch.full((nbytes,), 0xFF, device="cuda", dtype=torch.uint8)


@DTYPES
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("case", D.POISON_CASES)
def test_sampling_loops_do_not_read_uninitialised_workspace(case, cell, bf16):
    """The callers hand st_rnn_sample and st_rnn_sched_inputs a torch.empty workspace.  Here it is the caller's own, of exactly
    st_rnn_sample_workspace_bytes, every byte 0xFF: NaN in the fp32 logits (the pad columns of the pitch among them) and in the
    states of either dtype, -1 in the row's last token (`cur`; st_embedding_rows clamps an id, and the sampling kernel writes `cur`
    for every row before it is read), 255 in the <end> flags, which st_rnn_sample clears itself.  The ids and logp are those of the
    plain call, bit for bit."""
    from showtell_amd._lib import check, lib
    from showtell_amd.rnn import _cp, _stream
    c = D.CASES[case]
    m = _model(case, cell, bf16)
    assert D.paths(case)["pad_columns"] > 0
    prm, keep = m._c_params()
    feat_rows, u = D.sample_rows(case, cell, bf16)
    n, T = u.shape
    nbytes = lib().st_rnn_sample_workspace_bytes(C.byref(prm), n)
    assert nbytes == D.sample_plan(cell, bf16, c["E"], c["H"], c["L"], c["V"], n)[1]
    ids0, logp0, _ = _sample(m, case, cell, bf16, 0, 1.0)
    fr, ud = m._feature(feat_rows.cuda()), u.cuda().contiguous()
    ws = _poisoned(nbytes)
    ids = torch.full((n, T), -1, device="cuda", dtype=torch.long)
    logp = torch.full((n, T), float("nan"), device="cuda")
    check(lib().st_rnn_sample(C.byref(prm), _cp(fr), n, T, _cp(ud), 1.0, 0, D.END, _cp(ws), nbytes, _cp(ids), _cp(logp), _stream()), "st_rnn_sample")
    assert torch.equal(ids.cpu(), ids0) and torch.equal(logp.cpu().view(torch.int32), logp0.view(torch.int32)), _tag(case, cell, bf16)
    # the roll-in
    cap, lens, us = D.sched_problem(case)
    B, Tc = cap.shape
    ids0, rep0 = m.scheduled_inputs(_feat(case, cell, bf16), cap.cuda(), lens, D.SCHED_P, uniforms=us.cuda())
    nbytes = lib().st_rnn_sched_inputs_workspace_bytes(C.byref(prm), B)
    fb, capd, usd = m._feature(_feat(case, cell, bf16)), cap.cuda().contiguous(), us.cuda().contiguous()
    lensd = torch.tensor(lens, dtype=torch.int32, device="cuda")
    runs = []
    for ws in (torch.zeros(nbytes, device="cuda", dtype=torch.uint8), _poisoned(nbytes)):
        ids = torch.full((B, Tc), -1, device="cuda", dtype=torch.long)
        rep = torch.full((B, Tc), 7, device="cuda", dtype=torch.uint8)
        drawn = torch.full((B, Tc), -7, device="cuda", dtype=torch.long)
        logp = torch.full((B, Tc), float("nan"), device="cuda")
        check(lib().st_rnn_sched_inputs(C.byref(prm), _cp(fb), B, _cp(capd), Tc, _cp(lensd), max(lens), _cp(usd[0]), _cp(usd[1]), D.SCHED_P, 1.0,
                                        0, _cp(ws), nbytes, _cp(ids), _cp(rep), _cp(drawn), _cp(logp), _stream()), "st_rnn_sched_inputs")
        runs.append((ids.cpu(), rep.cpu(), drawn.cpu(), logp.cpu().view(torch.int32)))
    for a, b in zip(*runs):
        assert torch.equal(a, b), _tag(case, cell, bf16)
    assert torch.equal(runs[1][0], ids0.cpu()) and torch.equal(runs[1][1].bool(), rep0.cpu())
    assert torch.isfinite(runs[1][3].view(torch.float32)).all()


# ====================================================================================================================
# 6. refusals
# ====================================================================================================================

def _valid_call_still_passes(cell, bf16):
    ids, logp, lengths = _sample(_model("v_tiny", cell, bf16), "v_tiny", cell, bf16, 0, 1.0)
    D.judge_sample(ids, logp, lengths, "v_tiny", cell, bf16, 0, 1.0, "6 after a refusal")


@DTYPES
@pytest.mark.parametrize("cell", CELLS)
def test_top_k_above_the_vocabulary_is_a_value_error(cell, bf16):
    """check_sample_args / check_scheduled_args (rnn.py) refuse it in Python, before anything touches the device"""
    m, f = _model("v_tiny", cell, bf16), _feat("v_tiny", cell, bf16)
    V = D.CASES["v_tiny"]["V"]
    cap, lens = D.Y.captions([3] * 7, V, 3)
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match=f"1..{V}"):
        m.sample(f, 2, 1.0, V + 1, D.SAMPLE_T)
    with pytest.raises(ValueError, match=f"1..{V}"):
        m.sample(f, 2, 1.0, V + 1, D.SAMPLE_T, top_p=D.TOP_P)
    with pytest.raises(ValueError, match=f"1..{V}"):
        m.scheduled_inputs(f, cap.cuda(), lens, D.SCHED_P, top_k=V + 1)
    m.sample(f, 2, 1.0, V, D.SAMPLE_T)                             # top_k = V is the whole vocabulary: legal
    torch.cuda.synchronize()
    _valid_call_still_passes(cell, bf16)


@DTYPES
@pytest.mark.parametrize("cell", CELLS)
def test_width_9_leaves_the_device_selection(cell, bf16):
    """W * min(W, V) = 81 > 64: beam_search_records is refused by st_beam_select (a ShowTellHipError that names the limit) and
    beam_search is beam_search_host by itself; at V = 5 the same width is 45 candidates and stays on the device"""
    from showtell_amd import ShowTellHipError
    from showtell_amd.beam import beam_search_host, beam_search_records, replay_hypotheses
    m, f = _model("e_wider", cell, bf16), _feat("e_wider", cell, bf16)
    assert not D.paths("e_wider", 9)["on_device"] and D.paths("v_tiny", 9)["on_device"]
    with pytest.raises(ShowTellHipError, match="W \\* k <= 64"):
        beam_search_records(m, f, 9, D.BEAM_T)
    torch.cuda.synchronize()
    hyps = m.beam_search(f, 9, 2, D.BEAM_T)
    assert hyps == beam_search_host(m, f, 9, 2, D.BEAM_T) and any(hyps)
    for hyp in hyps:
        for s, cost in hyp:
            assert s[0] == D.START and s[-1] == D.END and all(0 <= v < D.CASES["e_wider"]["V"] for v in s) and np.isfinite(cost)
    mt, ft = _model("v_tiny", cell, bf16), _feat("v_tiny", cell, bf16)
    rec = beam_search_records(mt, ft, 9, D.BEAM_T)
    assert mt.beam_search(ft, 9, 1, D.BEAM_T) == replay_hypotheses(rec["tok"], rec["cost"], rec["par"], rec["end"], 1)
    _valid_call_still_passes(cell, bf16)


@DTYPES
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("E,H", [(12, 16), (16, 20), (12, 20)])
def test_scheduled_inputs_refuses_widths_that_are_no_multiple_of_8(E, H, cell, bf16):
    """st_rnn_step's check returns its error ahead of the first cell kernel (tests/test_gpu_decoder_geometry.py covers loss,
    sentence_index, beam_search and sample)"""
    from oracle import restatement as R
    from showtell_amd import ShowTellHipError
    m = _decoder(cell, R.init_decoder_params(E, H, D.Y.V, 2, cell, seed=5), _dtype(bf16), E, H, D.Y.V, 2).eval()
    feat = torch.randn(3, E, generator=torch.Generator().manual_seed(5)).cuda()
    cap, lens = D.Y.captions([4, 3, 2], D.Y.V, 5)
    torch.cuda.synchronize()
    with pytest.raises(ShowTellHipError, match="must be multiples of 8") as e:
        m.scheduled_inputs(feat, cap.cuda(), lens, D.SCHED_P)
    assert f"H={H}" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    _valid_call_still_passes(cell, bf16)
