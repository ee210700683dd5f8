"""CPU side of tests/test_gpu_decoding_geometry.py: that each case of tests/_decoding_geometry_cases.py takes the launch path it is
named for, that its inputs carry a signal, that the judges of the GPU test reject a decoder with a wrong stride, pitch, gather or
selection, and that every recorded floor is the one computed here.  Nothing here needs a GPU; two tests load the built library for
host-only planner calls, as tests/test_decoder_workspace.py does.

Measured here (float64 oracle alone, both cells and dtypes unless said):
  signal   every image of every beam case harvests a hypothesis within 8 steps (v2049: <end> boosted by 5.5, see the case table);
           the unfiltered samples hold 4 to 5 (v_tiny, V = 5), 8 to 9 (e_wider, V = 12) and 14 to 91 distinct tokens elsewhere, and 7 of
           18 (v2049) to all rows end; the roll-ins replace 10 of 19 (e_wider), 50 of 106 (h200), 20 of 35 (v2049) valid slots
  gap      steps of the filtered oracle's own draws whose top_k-th and next entry lie within the gap: fp32 at most 0.004 (tall_beam gru)
  faults   every (judge, case) of D.AIMED rejects its fault in both cells and dtypes
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _decoder_geometry_cases as Y
from tests import _decoding_geometry_cases as D
from tests import _scheduled_sampling_cases as K
from tests import test_sample_inputs as I

CELLS = list(D.CELLS)
DTYPES = pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
STALE = 0.006           # a recorded floor holds three digits


# ---- the paths -----------------------------------------------------------------------------------------------------------------

def test_cases_take_the_paths_they_are_named_for():
    p = {(c, W): D.paths(c, W) for c in D.CASES for W in D.CASES[c]["W"]}
    assert all(q["on_device"] and q["candidates"] <= 64 for q in p.values())
    # e_wider: in0 > H, the general top-k form at both widths (V = 12 < k * 256), four pad columns, a partial unit tile
    for W in (4, 8):
        q = p[("e_wider", W)]
        assert q["in0_wider"] and q["topk"] == "general" and q["k"] == W and (q["pitch"], q["pad_columns"]) == (16, 4)
        assert q["last_unit_tile"] == 8 and q["chunks"] == 3 and q["pitch"] == q["train_pitch"]
    assert [c for c in D.CASES if D.paths(c)["in0_wider"]] == ["e_wider"]
    # h200: 25 chunks per gathered row, a half-full last unit tile, ragged rows (37 images: 148 and 296 rows, no multiple of 16)
    q = p[("h200", 8)]
    assert q["chunks"] == 25 and q["last_unit_tile"] == 8 and D.CASES["h200"]["B"] == 37 and q["beam_tiles"] == (1, 19)
    assert p[("h200", 4)]["beam_tiles"] == (1, 10) and 37 * 4 % 16 and 37 * 8 % 16
    # h520: the first width past 512: 65 chunks, a partial unit tile
    q = p[("h520", 4)]
    assert D.CASES["h520"]["H"] == 520 and q["chunks"] == 65 and q["last_unit_tile"] == 8
    # v2049: the decoding pitch is up8(V) = 2056, training's 2560; the threshold top-k form up to W = 8 (8 * 256 = 2048 <= 2049);
    # the register sampling route
    for W in (4, 8):
        q = p[("v2049", W)]
        assert (q["pitch"], q["train_pitch"], q["pad_columns"]) == (2056, 2560, 7) and q["topk"] == "threshold" and q["sample_route"] == "regs"
    assert [c for c in D.CASES if D.paths(c)["pitch"] != D.paths(c)["train_pitch"]] == ["v2049"]
    assert [c for (c, W), q in p.items() if q["topk"] == "threshold"] == ["v2049", "v2049"]
    assert Y.up8(2048) == Y.vocab_ld(2048) == 2048 and D.paths("v2049", 9)["topk"] == "general"
    # v_tiny: k = V = 5 < W = 8, 40 candidates per image; at W = 4 k = W
    q = p[("v_tiny", 8)]
    assert (q["k"], q["candidates"], q["pad_columns"]) == (5, 40, 3) and p[("v_tiny", 4)]["k"] == 4 and D.TOP_K <= D.CASES["v_tiny"]["V"]
    # tall_beam: 520 rows per beam step and per sampling step: the two-row-tile cell kernel, taken from 512 rows on; no other case
    q = p[("tall_beam", 4)]
    assert q["beam_tiles"] == (2, 17) and q["sample_tiles"] == (2, 17) and 130 * 4 == 520
    assert [cw for cw, q in p.items() if q["beam_tiles"][0] == 2] == [("tall_beam", 4)]
    assert [c for c in D.CASES if D.paths(c)["sample_tiles"][0] == 2] == ["tall_beam"]
    assert Y.gemm_launch_tiles(1, 511)[0] == 1 and Y.gemm_launch_tiles(1, 512)[0] == 2
    # every case samples on the register route (V <= 256 * 40 and a pitch of 8 | 4): the memory routes are tests/test_gpu_sample.py's
    assert all(D.paths(c)["sample_route"] == "regs" for c in D.CASES)
    # W = 9: W * min(W, V) > 64 leaves the device selection for every vocabulary of 8 words or more
    assert not D.paths("e_wider", 9)["on_device"] and D.paths("v_tiny", 9)["on_device"]


@pytest.mark.parametrize("cell", CELLS)
def test_the_library_plans_the_sampling_workspace_as_the_mirror_does(cell):
    """host-only (it loads the built library): st_rnn_sample_workspace_bytes and st_rnn_sched_inputs_workspace_bytes to the byte, x at
    n * E beside states of L * n * H, logits at pitch up8(V)"""
    from showtell_amd._lib import lib
    from tests.test_decoder_workspace import _rnn_params
    for case, c in D.CASES.items():
        for bf16 in (False, True):
            p = _rnn_params(cell, "bf16" if bf16 else "f32", c["E"], c["E"], c["H"], c["L"], c["V"])
            for n in (c["B"], c["B"] * c["S"]):
                want = D.sample_plan(cell, bf16, c["E"], c["H"], c["L"], c["V"], n)[1]
                assert lib().st_rnn_sample_workspace_bytes(C.byref(p), n) == want, (case, bf16, n)
                assert lib().st_rnn_sched_inputs_workspace_bytes(C.byref(p), n) == want, (case, bf16, n)


# ---- signal --------------------------------------------------------------------------------------------------------------------

@DTYPES
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("case", list(D.CASES))
def test_the_oracle_alone_shows_that_the_inputs_carry_a_signal(case, cell, bf16):
    c = D.CASES[case]
    for W in c["W"]:
        rec = D.oracle_records(case, cell, bf16, W)
        assert rec["end"].any((0, 2)).all(), (W, "every image harvests a hypothesis within 8 steps")
        assert np.isfinite(rec["cost"][-1]).any(), (W, "some image is still searched at the last step")
    ids, _, lp = D.oracle_samples(case, cell, bf16)
    m = I.checked_mask(ids)
    ended = int((ids == D.END).any(1).sum())
    print(f"MEASURE signal {case} {cell} bf16={bf16}: distinct tokens {ids[m].unique().numel()}, rows ended {ended} of {ids.shape[0]}")
    assert ids[m].unique().numel() >= min(6, c["V"] - 1) and ended >= 1
    assert (ids[:, 0] != D.END).any(), "not every row ends at once"
    if c["sched"]:
        out, rep, _ = D.oracle_roll_in(case, cell, bf16)
        cap, lens, _ = D.sched_problem(case)
        valid = int(K.valid_slots("rnn", lens, cap.shape[1]).sum())
        assert 0.4 * valid <= int(rep.sum()) <= 0.6 * valid, (int(rep.sum()), valid)
        assert int((out != cap).sum()) >= 0.8 * int(rep.sum()), "a replaced slot usually holds another token than the caption's"
        assert any(l == 1 for l in lens) or case == "h200", "a row without a slot to replace"


@pytest.mark.parametrize("cell", CELLS)
def test_the_filtered_fp32_oracle_leaves_few_steps_within_the_top_k_gap(cell, bf16=False):
    """in fp32 judge_sample leaves out a step whose top_k-th and next log-probability lie within Y.FP32_GAP and allows EXCLUDED of the
    steps to be such: the oracle's own filtered draws stay under that share in every case.  (bf16 leaves nothing out: within its
    gap, 4 x the storage floor of a log-probability, lie up to a fifth of the steps, and those are judged against either set.)"""
    for case, c in D.CASES.items():
        if D.TOP_K >= c["V"]:
            continue
        ids, _, lp = D.oracle_samples(case, cell, bf16, D.TOP_K, D.TOP_P)
        m = I.checked_mask(ids)
        within = int((D.kth_gap(lp, D.TOP_K) <= D.topk_gap(case, cell, bf16))[m].sum())
        print(f"MEASURE gap {case} {cell} bf16={bf16}: {within} of {int(m.sum())} steps within {D.topk_gap(case, cell, bf16):.2e}")
        assert within <= D.EXCLUDED * int(m.sum()), (case, within, int(m.sum()))


def test_the_fp32_scale_is_that_of_the_logits():
    """FP32_REL is a share of the tensor's scale: max |logit| along the float64 oracle's own samples"""
    for case in D.CASES:
        for cell in CELLS:
            s = D.logit_scale(case, cell)
            assert 3.0 < s < 12.0, (case, cell, s)
            assert D.beam_bound(case, cell, False) == D.FP32_REL * s == D.sample_bounds(case, cell, False)[1]


# ---- the judges: the clean oracle passes, the seeded faults do not ------------------------------------------------------------------

def _lengths(ids):
    return I.checked_mask(ids).sum(1)


def _judged(kind, case, cell, bf16, fault):
    """the findings of the judge `kind` on the faulty oracle's own output: a list of AssertionErrors (empty: it passes)"""
    out = []

    def attempt(fn, *a, **kw):
        try:
            fn(*a, **kw)
        except AssertionError as e:
            out.append(e)
    if kind == "beam":
        for W in D.CASES[case]["W"]:
            attempt(D.judge_beam, D.oracle_records(case, cell, bf16, W, fault), case, cell, bf16, W, f"{fault} W={W}")
    elif kind == "sample":
        for top_k, top_p in ((0, 1.0), (D.TOP_K, D.TOP_P)):
            ids, logp, _ = D.oracle_samples(case, cell, bf16, top_k, top_p, fault)
            attempt(D.judge_sample, ids, logp, _lengths(ids), case, cell, bf16, top_k, top_p, f"{fault} top_k={top_k}")
    else:
        ids, rep, _ = D.oracle_roll_in(case, cell, bf16, fault)
        attempt(D.judge_sched, ids, rep, case, cell, bf16, fault)
    return out


def _kinds(case):
    return ("beam", "sample") + (("sched",) if D.CASES[case]["sched"] else ())


@DTYPES
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("case", list(D.CASES))
def test_every_judge_accepts_the_oracle_itself(case, cell, bf16):
    for kind in _kinds(case):
        assert _judged(kind, case, cell, bf16, None) == [], (kind, case)


def _reaches(fault, case):
    c = D.CASES[case]
    return {"x_pitch_h": c["E"] != c["H"], "unit_tail_lost": c["H"] % 64 != 0,
            "logits_pitch_train": Y.up8(c["V"]) != Y.vocab_ld(c["V"])}.get(fault, True)


@DTYPES
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("fault", D.FAULTS)
def test_seeded_fault_is_rejected_where_it_is_aimed(fault, cell, bf16):
    assert D.AIMED[fault], "a fault no judge catches on any case means the cases are too weak"
    for kind, case in D.AIMED[fault]:
        assert _reaches(fault, case) and kind in _kinds(case)
        found = _judged(kind, case, cell, bf16, fault)
        print(f"MEASURE fault {fault} {kind} {case} {cell} bf16={bf16}: {len(found)} findings")
        assert found, (fault, kind, case, cell, "the judge accepts the faulty decoder")


@pytest.mark.parametrize("fault", ["x_pitch_h", "unit_tail_lost", "logits_pitch_train"])
def test_a_fault_of_the_step_leaves_the_cases_it_cannot_reach(fault):
    """x_pitch_h is invisible at E = H, logits_pitch_train below V = 2048, unit_tail_lost at a multiple of 64: why the widths and
    vocabularies of the other decoding tests cannot see them"""
    reach = [c for c in D.CASES if _reaches(fault, c)]
    assert reach == {"x_pitch_h": ["e_wider"], "unit_tail_lost": ["e_wider", "h200", "h520", "v_tiny", "tall_beam"],
                     "logits_pitch_train": ["v2049"]}[fault]
    for case in D.CASES:
        if case in reach:
            continue
        a, b = D.oracle_samples(case, "gru", True, 0, 1.0, fault), D.oracle_samples(case, "gru", True)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), (fault, case)


# ---- floors --------------------------------------------------------------------------------------------------------------------

def _fresh(got, rec):
    return abs(got - rec) <= STALE * rec


def test_recorded_floors_are_the_computed_ones():
    """the bf16 bounds are 4 x these: the float64 oracle against its bf16-storage replica on the bf16-representable inputs, along
    the replica's own search, draws and roll-in"""
    keys = [(case, cell) for case in D.CASES for cell in CELLS]
    assert list(D.BEAM_FLOORS) == keys and list(D.SAMPLE_FLOORS) == keys
    assert list(D.SCHED_FLOORS) == [(case, cell) for case in D.SCHED_CASES for cell in CELLS]
    for key in keys:
        got = D.beam_floor(*key)
        assert _fresh(got, D.BEAM_FLOORS[key]), ("beam", key, got)
        got = D.sample_floor(*key)
        assert all(_fresh(g, r) for g, r in zip(got, D.SAMPLE_FLOORS[key])), ("sample", key, got)
        # a bound of use: storage moves a log-probability by a few hundredths at most, the seeded faults by far more (above)
        assert 4 * D.BEAM_FLOORS[key] < 0.1 and 4 * D.SAMPLE_FLOORS[key][1] < 0.1 and 4 * D.SAMPLE_FLOORS[key][0] < 0.01, key
    for key in D.SCHED_FLOORS:
        got = D.sched_floor(*key)
        assert _fresh(got, D.SCHED_FLOORS[key]), ("sched", key, got)
        assert 4 * D.SCHED_FLOORS[key] < 0.01, key
