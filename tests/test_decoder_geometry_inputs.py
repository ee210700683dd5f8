"""The inputs of tests/test_gpu_decoder_geometry.py, checked on the CPU (tests/_decoder_geometry_cases.py): the cases take the launch
paths they are named for, their gradients carry signal, every seeded fault of a launch that mishandles a width, a vocabulary or a
batch shape moves a compared quantity beyond twice its bound on the cases it is aimed at (and by nothing on the cases it cannot
reach), and the floors the GPU bounds are read from are the recorded ones.

Printed with -s (MEASURE ...).  Measured here:
  signal     smallest max |d W| of a layer over the largest gradient element of its model: 2.3e-2 (tall_single gru); bound 1e-3
  faults     the smallest margin of a seeded fault on a case it is aimed at: 4.4 bounds (split_slice_lost, v2047 lstm) among the
             gradients, and pad_columns_in_softmax on v2049 by the loss (4.5 and 5.3 x LOSS_REL; its gradients move by 2.3 and 1.4
             bounds: 511 zero logits beside 2049 real ones weigh a fifth of the softmax, spread evenly); bound 2; every case a
             fault cannot reach is unmoved to the last bit
  greedy     fp32 against float64 arithmetic moves a logit by at most 4.4e-6 (gru, h256) and 2.8e-6 (lstm, h256); no step of any
             float64 walk has a top-two gap within 4 x that (smallest gap 1.2e-4, h200 lstm); the bf16 storage restatement in fp32
             arithmetic keeps every row of every case but one of h200 lstm's 37 (gap 1.5e-3 of max |logit|): DELTA and AGREE hold
  floors     STORAGE_FLOORS: bf16 storage alone reaches a quarter of the project's bounds only on e_wider (five tokens, H = 24)
The whole file takes a few seconds.
"""
import pytest
import torch

from tests import _decoder_geometry_cases as Y
from tests.test_gpu_decoder_bench_shape import AGREE, DELTA, LOSS_REL

CELLS = list(Y.CELLS)
SIGNAL = 1e-3       # every layer's largest weight-gradient element over the model's largest gradient element (the depth suite's)
FAULT_MARGIN = 2.0  # a fault moves some compared quantity by at least this many bounds on the cases it is aimed at


# ---- the paths -----------------------------------------------------------------------------------------------------------------

def test_vocab_ld_and_the_dy_split_follow_the_planner():
    assert [Y.vocab_ld(v) for v in (1, 12, 50, 2047, 2048, 2049, 10000)] == [8, 16, 56, 2048, 2048, 2560, 10240]
    for bf16 in (True, False):
        assert Y.dy_split(2048, bf16) == 8 and Y.dy_split(2560, bf16) == 8 and Y.dy_split(56, bf16) == 0
    assert Y.dy_split(1024, True) == 8 and Y.dy_split(512, True) == 0 and Y.dy_split(512, False) == 8 and Y.dy_split(256, False) == 0
    assert Y.dy_split(1536, True) == 8 and Y.dy_split(1280, True) == 0 and Y.dy_split(1280, False) == 8


def test_the_library_agrees_on_vocab_ld():
    """host-only (it loads the built library, as tests/test_decoder_workspace.py does)"""
    from showtell_amd._lib import lib
    for v in (1, 7, 8, 12, 50, 2040, 2041, 2047, 2048, 2049, 2560, 2561, 10000):
        assert lib().st_rnn_vocab_ld(v) == Y.vocab_ld(v), v


@pytest.mark.parametrize("cell", CELLS)
def test_cases_take_the_paths_they_are_named_for(cell):
    G = 3 if cell == "gru" else 4
    p = {(case, bf16): Y.paths(case, cell, bf16) for case in Y.CASES for bf16 in (True, False)}
    for (case, bf16), q in p.items():
        assert not q["fused_ce"] and not q["pipe"], case              # no case has H = 512: both must decline
        assert q["tn_route"] == bf16

    # e_wider: in0 > H
    for bf16 in (True, False):
        q = p[("e_wider", bf16)]
        assert q["maxw"] == 72 > Y.CASES["e_wider"]["H"] and q["dx0_tile"] == "wide"
        assert q["vocab_ld"] == 16 and q["pad_columns"] == 4 and q["dy_split"] == 0
        assert q["tn"][1] == ("unit.weight_ih_l0", G * 24, 72, 1, 1, G * 24, 72)           # its own descriptor with N = 72
        assert all(d[2] == 24 for d in q["tn"] if d[0] != "unit.weight_ih_l0")
        assert q["last_unit_tile"] == 8
        assert q["diagonals"] == [(1, 5, 1), (2, 5, 1), (2, 5, 1), (2, 3, 1), (1, 2, 1)]
    q = p[("e_wider", True)]
    assert q["fwd_steps"]["recurrent"] == ([1, 0, 0, 0], 24)         # K = 24: less than one bf16 step, three waves without one
    assert q["fwd_steps"]["input0"] == ([1, 1, 1, 0], 8)             # K2 = 72: two steps and a quarter
    assert q["fwd_steps"]["input"] == ([1, 0, 0, 0], 24)
    assert p[("e_wider", False)]["fwd_steps"]["input0"] == ([2, 2, 1, 0], 8)

    # h200: H no multiple of 16 or 32, two gemm_tn column tiles with a 72-column tail, the generic arg-max in both dtypes
    for bf16 in (True, False):
        q = p[("h200", bf16)]
        assert q["last_unit_tile"] == 8 and q["bwd_blocks"] == (2, 7) and q["maxw"] == 200
        assert q["tn"][0] == ("linear.weight", 50, 200, 1, 2, 50, 72)
        rows = G * 200
        assert all(d[1:] == (rows, 200, -(-rows // 128), 2, rows - 128 * (rows // 128), 72) for d in q["tn"][1:]) and len(q["tn"]) == 5
        assert q["argmax"][0] == "generic"
        assert q["diagonals"] == [(1, 37, 1), (2, 37, 2), (2, 37, 2), (2, 33, 2), (2, 17, 2), (2, 16, 1), (1, 3, 1)]
    assert p[("h200", True)]["fwd_steps"]["recurrent"] == ([2, 2, 2, 1], 8)
    assert p[("h200", True)]["bwd_steps"]["recurrent"] == (([5, 5, 5, 4], 24) if cell == "gru" else ([7, 7, 7, 4], 0))
    assert p[("h200", False)]["fwd_steps"]["recurrent"] == ([4, 4, 4, 1], 8)

    # h520: the first width past 512
    for bf16 in (True, False):
        q = p[("h520", bf16)]
        assert q["tn"][0] == ("linear.weight", 50, 520, 1, 5, 50, 8)                       # four full column tiles and one 8-column chunk
        assert all(d[4:] == (5, (G * 520) % 128, 8) for d in q["tn"][1:])
        assert q["argmax"][0] == "generic" and q["last_unit_tile"] == 8 and q["bwd_blocks"] == (1, 17)
        assert Y.pipe_eligible(512, 512, 2, Y.V, 5, True) and not q["pipe"]                # 512 would be eligible in bf16
    assert p[("h520", True)]["fwd_steps"]["recurrent"] == ([5, 5, 5, 2], 8)

    # h256: the LDS-staged arg-max at a width other than 64, 128 or 512; the fp32 form's widest
    assert p[("h256", True)]["argmax"] == ("lds", 48, 1) and p[("h256", False)]["argmax"] == ("lds", 48, 1)
    assert Y.argmax_route(288, Y.V, 33, False)[0] == "generic" and Y.argmax_route(544, Y.V, 33, True)[0] == "generic"
    assert Y.argmax_route(224, Y.V, 33, True)[0] == "generic"                               # bf16 widths go in steps of 64

    # v2047 / v2049: either side of the rounding rule, 8 K slices in both dtypes
    for bf16 in (True, False):
        a, b = p[("v2047", bf16)], p[("v2049", bf16)]
        assert (a["vocab_ld"], a["pad_columns"], a["dy_split"], a["last_slice"]) == (2048, 1, 8, (1792, 2048))
        assert (b["vocab_ld"], b["pad_columns"], b["dy_split"], b["last_slice"]) == (2560, 511, 8, (2240, 2560))
        assert a["last_slice"][0] < 2047 < a["last_slice"][1]          # one pad column inside the last slice
        assert b["last_slice"][0] >= 2049                              # the last slice is nothing but padding
        assert a["dx0_tile"] == b["dx0_tile"] == "128x64"              # N = in0 = 64
        assert a["tn"][0][3:] == (16, 1, 127, 64) and b["tn"][0][3:] == (17, 1, 1, 64)
        assert a["argmax"][0] == "lds"

    # tall_single / mid_single: one cell per launch
    for bf16 in (True, False):
        q = p[("tall_single", bf16)]
        assert q["diagonals"] == [(1, 520, 2), (1, 513, 2)]           # nc = 1 and maxM >= 512: two row tiles per block
        assert q["bwd_blocks"] == (17, 1) and (q["ntok"], q["Np"]) == (1033, 1040)
        q = p[("mid_single", bf16)]
        assert q["diagonals"] == [(1, 37, 1), (1, 37, 1), (1, 33, 1), (1, 17, 1), (1, 16, 1), (1, 3, 1)]
        assert Y.gemm_launch_tiles(1, 37) == (1, 3) and Y.gemm_launch_tiles(1, 511) == (1, 32) and Y.gemm_launch_tiles(1, 512) == (2, 16)
    assert Y.gemm_launch_tiles(2, 16) == (1, 1) and Y.gemm_launch_tiles(2, 17) == (2, 1)


def test_e_is_at_most_h_in_every_case_but_e_wider():
    assert [c for c, v in Y.CASES.items() if v["E"] > v["H"]] == ["e_wider"]
    assert set(Y.ROUTE_CASES) | set(Y.POISON_CASES) <= set(Y.TRAIN_CASES) and "h256" in Y.GREEDY_CASES


# ---- signal --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("case", Y.TRAIN_CASES)
def test_every_layer_has_a_gradient_worth_comparing(case, cell):
    for bf16 in (False, True):
        g = Y.grads(case, cell, bf16)[2]
        big = max(v.abs().max().item() for v in g.values())
        s, k = min((g[k].abs().max().item() / big, k) for k in g if "unit.weight" in k)
        print(f"MEASURE signal {case} {cell} {'bf16' if bf16 else 'fp32'}: {s:.2e} ({k})")
        assert s >= SIGNAL, (case, cell, k, s)
        assert all(torch.isfinite(v).all() for v in g.values())


# ---- seeded faults -------------------------------------------------------------------------------------------------------------

def _margin(case, cell, fault):
    """the largest (distance / bound) over the compared quantities -- every gradient and dfeat in both norms, the loss, token_logp --
    with the bf16 bounds on the bf16 inputs (the fp32 bound, 2e-4 of the tensor's scale, is tighter than every one of them)"""
    ref, got = Y.grads(case, cell, True), Y.grads(case, cell, True, fault)
    worst = (abs(got[0] - ref[0]) / abs(ref[0]) / LOSS_REL, "loss")
    for k, (l2, mx) in Y.distance(got[2], ref[2]).items():
        bl2, bmx = Y.bf16_bounds(case, cell, k)
        worst = max(worst, (l2 / bl2, k), (mx / bmx, k), key=lambda v: v[0])
    _, _, cap, lens = Y.problem(case, cell, True)
    l2, mx = Y.logp_distance(Y.token_logp(got[1], cap, lens), Y.token_logp(ref[1], cap, lens))
    bl2, bmx = Y.logp_bounds(case, cell)
    return max(worst, (l2 / bl2, "token_logp"), (mx / bmx, "token_logp"), key=lambda v: v[0])


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("case", Y.TRAIN_CASES)
@pytest.mark.parametrize("fault", Y.FAULTS)
def test_seeded_fault_is_caught_where_it_is_aimed_and_leaves_the_cases_it_cannot_reach(fault, case, cell):
    m, k = _margin(case, cell, fault)
    print(f"MEASURE fault {fault} {case} {cell}: {m:.2e} bounds ({k}); reaches {Y.reaches(fault, case)}, aimed {case in Y.AIMED[fault]}")
    if case in Y.AIMED[fault]:
        assert Y.reaches(fault, case) and m >= FAULT_MARGIN, (fault, case, cell, m, k)
    elif not Y.reaches(fault, case):
        assert m == 0.0, (fault, case, cell, m, k)


def test_fault_reach_is_as_the_cases_are_meant():
    reach = {f: [c for c in Y.TRAIN_CASES if Y.reaches(f, c)] for f in Y.FAULTS}
    assert reach["last_unit_tile_lost"] == ["e_wider", "h200", "h520"]
    assert reach["k_tail_dropped"] == ["e_wider", "h200", "h520", "tall_single", "mid_single"]
    assert reach["wave_without_steps_reads_on"] == ["e_wider", "v2047", "v2049", "tall_single", "mid_single"]
    assert reach["pad_columns_in_softmax"] == list(Y.TRAIN_CASES)
    assert reach["split_slice_lost"] == ["v2047"]                     # v2049's last slice holds no vocabulary column
    assert reach["tn_column_tail_lost"] == list(Y.TRAIN_CASES)
    assert reach["rows_from_512_lost"] == ["tall_single"]
    assert reach["wide_input_truncated"] == ["e_wider"]
    assert sorted(Y.AIMED) == sorted(Y.FAULTS) and all(set(Y.AIMED[f]) <= set(reach[f]) for f in Y.FAULTS)


# ---- bf16 storage floors -------------------------------------------------------------------------------------------------------

def test_recorded_storage_floors_are_the_computed_ones():
    """Y.STORAGE_FLOORS holds exactly the gradients that bf16 storage alone moves by a quarter of the project's bound or more, with
    the distances computed here (float64 on both sides: to the three digits recorded)"""
    got = {}
    for case in Y.TRAIN_CASES:
        for cell in CELLS:
            for k, (l2, mx) in Y.storage_distance(case, cell).items():
                pl2, pmx = Y.project_bounds(k)
                print(f"MEASURE floor {case} {cell} {k}: rel_l2 {l2:.2e} rel_max {mx:.2e} (project bounds {pl2:.0e}, {pmx:.0e})")
                if l2 >= pl2 / 4 or mx >= pmx / 4:
                    got[(case, cell, k)] = (l2, mx)
    for key, v in sorted(got.items()):
        print(f"    {key!r}: ({v[0]:.2e}, {v[1]:.2e}),")
    assert sorted(got) == sorted(Y.STORAGE_FLOORS), sorted(set(got) ^ set(Y.STORAGE_FLOORS))
    for key, (l2, mx) in got.items():
        rl2, rmx = Y.STORAGE_FLOORS[key]
        assert abs(l2 - rl2) <= 0.006 * rl2 and abs(mx - rmx) <= 0.006 * rmx, (key, (l2, mx), (rl2, rmx))


def test_recorded_logp_floors_are_the_computed_ones():
    got = {}
    for case in Y.TRAIN_CASES:
        for cell in CELLS:
            l2, mx = Y.logp_distance(Y.oracle_logp(case, cell, True, True), Y.oracle_logp(case, cell, True))
            print(f"MEASURE floor token_logp {case} {cell}: rel_l2 {l2:.2e} rel_max {mx:.2e}")
            if l2 >= Y.GRAD_L2 / 4 or mx >= Y.GRAD_MAX / 4:
                got[(case, cell)] = (l2, mx)
    assert sorted(got) == sorted(Y.LOGP_FLOORS), got
    for key, (l2, mx) in got.items():
        rl2, rmx = Y.LOGP_FLOORS[key]
        assert abs(l2 - rl2) <= 0.006 * rl2 and abs(mx - rmx) <= 0.006 * rmx, (key, (l2, mx), (rl2, rmx))


# ---- greedy decoding -------------------------------------------------------------------------------------------------------------

def test_recorded_fp32_gap_is_the_computed_one_and_the_walks_leave_few_steps_within_it():
    """an fp32 token is compared with the float64 walk wherever that walk's top-two gap exceeds Y.FP32_GAP: the gap is 4 x what fp32
    arithmetic alone moves a logit by (to a factor of 2: another CPU's fp32 sums differ), and the float64 walk of every case leaves at
    most Y.EXCLUDED of its steps within it"""
    for cell in CELLS:
        floor = max(Y.fp32_greedy_floor(case, cell) for case in Y.GREEDY_CASES)
        print(f"MEASURE floor fp32 greedy {cell}: |d logit| {floor:.3e}")
        assert Y.FP32_GAP[cell] / 2 <= 4 * floor <= Y.FP32_GAP[cell] * 2, (cell, floor, Y.FP32_GAP[cell])
        for case in Y.GREEDY_CASES:
            params, feat, _, _ = Y.problem(case, cell, False)
            lg, ids = Y.greedy_walk(params, feat, cell, False)
            gap = Y.top_two_gap(lg)
            within = int((gap <= Y.FP32_GAP[cell]).sum())
            print(f"MEASURE greedy {case} {cell} fp32: {within} of {gap.numel()} steps within the gap, smallest gap {gap.min().item():.2e}, "
                  f"{ids.unique().numel()} distinct tokens")
            assert within / gap.numel() <= Y.EXCLUDED, (case, cell, within)
            assert ids.unique().numel() >= 5, "the walk must not collapse to a constant token"


def test_bf16_greedy_restatement_in_fp32_arithmetic_against_the_greedy_bounds():
    """the GPU test holds the bf16 greedy ids to DELTA and AGREE, or to the looser pair where no fp32 implementation can be owed
    them: Y.GREEDY_LOOSE is exactly the set of (case, cell) at which the storage restatement in fp32 arithmetic misses them against
    its float64 self"""
    loose = []
    for case in Y.GREEDY_CASES:
        for cell in CELLS:
            share, gap = Y.plain_greedy_floor(case, cell)
            print(f"MEASURE floor bf16 greedy {case} {cell}: fp32 against float64 arithmetic agree on {share:.3f} of the rows, worst gap {gap:.2e}")
            if share < AGREE or gap > DELTA:
                loose.append((case, cell))
    assert sorted(loose) == sorted(Y.GREEDY_LOOSE), loose


@pytest.mark.parametrize("cell", CELLS)
def test_greedy_planner_reserves_no_pipeline_bytes_at_these_widths(cell):
    """host-only (it loads the built library): at H != 512 the greedy workspace is the launch chain's own buffers to the byte
    (greedy_chain_bytes of tests/_decoder_depth_cases.py, a mirror of make_greedy_plan without the pipelined decoder's region), in
    both dtypes; at E = H = 512 in bf16 the same depth and batch carry that region"""
    import ctypes as C

    from showtell_amd._lib import lib
    from tests._decoder_depth_cases import greedy_chain_bytes
    from tests.test_decoder_workspace import _rnn_params
    for case in Y.GREEDY_CASES:
        c = Y.CASES[case]
        B = len(c["lens"])
        for dtype, bf16 in (("bf16", True), ("f32", False)):
            p = _rnn_params(cell, dtype, c["E"], c["E"], c["H"], c["L"], c["V"])
            assert lib().st_rnn_greedy_workspace_bytes(C.byref(p), B) == greedy_chain_bytes(cell, bf16, c["E"], c["H"], c["L"], c["V"], B), (case, dtype)
    p = _rnn_params(cell, "bf16", 512, 512, 512, 2, Y.V)
    assert lib().st_rnn_greedy_workspace_bytes(C.byref(p), 5) > greedy_chain_bytes(cell, True, 512, 512, 2, Y.V, 5)
