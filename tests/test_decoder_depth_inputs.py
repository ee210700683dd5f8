"""The inputs of tests/test_gpu_decoder_depth.py, checked on the CPU (tests/_decoder_depth_cases.py): the cases take the launch paths
they are named for, their gradients carry signal through every layer, every seeded fault of a launch at depth moves a compared
quantity by at least 4 x its bound on every case it can reach (and by nothing on the others), and the bf16 storage floors the
GPU bounds are read from are the recorded ones.

Printed with -s (MEASURE ...).  Measured here:
  signal     smallest max |d W| of a layer over the largest gradient element of its model: plain 2.0e-3 (eight_wide lstm), attention
             1.35e-3 (eight_long lstm); bound 1e-3
  depth      replacing layer 0's output by zeros moves the top-two logit gap of the first five greedy steps, at the median, by at
             least 8.7e-3 of max |logit| (attention six lstm; attention eight_long lstm 8.9e-3) over the greedy cases of the plain and
             attention decoders and the beam inputs of both; bound 2^-7
  faults     the smallest margin of a seeded fault on a case it reaches: 53 bounds (carry_of_neighbour, seven_narrow lstm); bound 4;
             every case a fault cannot reach is unmoved to the last bit
  greedy     the float64 attention walk leaves 0.080 (gru) and 0.030 (lstm) of its bf16 steps within the gap (bound 0.09; the GPU
             test allows 0.10)
  floors     the tables of tests/_decoder_depth_cases.py are recomputed: float64 on both sides to the three digits recorded, those
             that fp32 arithmetic enters to a factor of 2 (another CPU's fp32 sums round a stored value the other way somewhere)
The whole file takes 15 s.
"""
import pytest
import torch

from oracle import restatement as R
from tests import _decoder_depth_cases as Z

CELLS = ["gru", "lstm"]
SIGNAL = 1e-3       # every layer's largest weight-gradient element over the model's largest gradient element
DEPTH_GAP = 2.0 ** -7    # change of the median top-two logit gap over max |logit| when layer 0's output is replaced by zeros on its way
                         # up: DELTA, the divergence tolerance of the bf16 greedy check (tests/test_gpu_decoder_bench_shape.py)
FAULT_MARGIN = 4.0  # a fault moves some compared tensor by at least this many bounds


# ---- the paths -----------------------------------------------------------------------------------------------------------------

def test_cases_take_the_paths_they_are_named_for():
    p = {case: Z.paths(case) for case in Z.CASES}
    assert [len(p[c]["descriptors"]) for c in Z.CASES] == [12, 13, 16, 16, 16]
    assert [p[c]["groups"] for c in Z.CASES] == [[12], [12, 1], [12, 4], [12, 4], [12, 4]]
    # seven_narrow: layer 0's dW_ih is not among the descriptors (a GEMM of its own), and the lone thirteenth is dW_hh of layer 6
    assert "unit.weight_ih_l0" not in p["seven_narrow"]["descriptors"] and p["seven_narrow"]["descriptors"][12] == "unit.weight_hh_l6"
    assert p["eight_long"]["descriptors"][12:] == [f"unit.weight_{w}_l{l}" for l in (6, 7) for w in ("ih", "hh")]
    assert p["eight_long"]["max_cells"] == 8 == Z.MAX_LAYERS
    assert p["eight_short"]["max_cells"] <= 2 and p["eight_short"]["late_start"]
    assert all(len(d) < 8 for d in p["eight_short"]["diagonals"])              # no diagonal holds every layer
    assert all(d[0] == i + 1 for i, d in enumerate(p["eight_short"]["diagonals"][2:]))   # every diagonal d >= T starts at d - (T - 1)
    assert p["six"]["max_cells"] == 4 and p["seven_narrow"]["max_cells"] == 5
    # every cell (l, t) is on exactly one diagonal
    for case, c in Z.CASES.items():
        cells = [(l, d - l) for d, ls in enumerate(p[case]["diagonals"]) for l in ls]
        assert sorted(cells) == [(l, t) for l in range(c["L"]) for t in range(c["lens"][0])], case
    # packed batch sizes of eight_long cross a 32-row and a 16-row tile, and the recurrent pair has fewer rows than the cell
    bs = R.batch_sizes(Z.CASES["eight_long"]["lens"])
    assert len(bs) == 10 and bs[0] == 37 and any(a > 32 >= b for a, b in zip(bs, bs[1:])) and any(a > 16 >= b for a, b in zip(bs, bs[1:]))
    c = Z.CASES["eight_wide"]
    assert not p["eight_wide"]["pipe"] and Z.pipe_eligible(c["E"], c["H"], 5, c["V"], len(c["lens"]), True)
    assert not any(p[case]["pipe"] for case in Z.CASES)
    assert c["H"] == 512 and len(c["lens"]) == 33 and sum(c["lens"]) == 86   # full 32 x 32 tiles plus the row tail


# ---- signal --------------------------------------------------------------------------------------------------------------------

def _signal(g):
    big = max(v.abs().max().item() for v in g.values())
    return min((g[k].abs().max().item() / big, k) for k in g if "unit.weight" in k)


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("case", list(Z.CASES))
def test_every_layer_has_a_gradient_worth_comparing(case, cell):
    for bf16 in (False, True):
        s, k = _signal(Z.grads(case, cell, bf16)[2])
        print(f"MEASURE signal plain {case} {cell} {'bf16' if bf16 else 'fp32'}: {s:.2e} ({k})")
        assert s >= SIGNAL, (case, cell, k, s)
        if case in Z.ATTN_CASES:
            s, k = _signal(Z.attn_grads(case, cell, bf16)[2])
            print(f"MEASURE signal attention {case} {cell} {'bf16' if bf16 else 'fp32'}: {s:.2e} ({k})")
            assert s >= SIGNAL, (case, cell, k, s)


def _greedy_gaps(params, feat, cell, damp, steps=5, tokens=None):
    """top-two logit gaps (B, steps) and max |logit| of the first greedy steps (R.rnn_greedy's loop), layer 0's output multiplied by
    `damp` on its way up (the recurrence keeps the plain one); fed `tokens` (B, steps) when given, its own arg-max otherwise"""
    L = R.num_layers_of(params)
    H = params["unit.weight_hh_l0"].shape[1]
    h = [feat.new_zeros(feat.shape[0], H) for _ in range(L)]
    c = [feat.new_zeros(feat.shape[0], H) for _ in range(L)]
    x, gaps, scales, ids = feat, [], [], []
    for t in range(steps):
        inp = x
        for l in range(L):
            w = R._layer_w(params, l)
            if cell == "gru":
                h[l] = R.gru_cell(inp, h[l], *w)
            else:
                h[l], c[l] = R.lstm_cell(inp, h[l], c[l], *w)
            inp = h[l] * damp if l == 0 else h[l]
        lg = inp @ params["linear.weight"].t() + params["linear.bias"]
        tv = torch.topk(lg, 2, dim=1)[0]
        gaps.append(tv[:, 0] - tv[:, 1]); scales.append(lg.abs().max(1)[0]); ids.append(lg.max(1)[1])
        x = params["embeddings.weight"][ids[-1] if tokens is None else tokens[:, t]]
    return torch.stack(gaps, 1), torch.stack(scales, 1), torch.stack(ids, 1)


def _attn_greedy_gaps(params, feat, cell, damp, steps=5, tokens=None):
    """the same for the attention decoders (R.attn_greedy's loop from <start>)"""
    B = feat.shape[0]
    h, c = R._attn_init(params, feat, cell)
    h, c = list(h), (list(c) if c is not None else [None] * len(h))
    fb = feat.transpose(1, 2)
    tok, gaps, scales, ids = torch.full((B,), 1, dtype=torch.long), [], [], []
    for t in range(steps):
        z, _ = R.attention_net(params, fb, h[-1])
        inp = torch.cat([params["embeddings.weight"][tok], z @ params["embed.weight"].t() + params["embed.bias"]], 1)
        for l in range(len(h)):
            w = R._layer_w(params, l)
            if cell == "gru":
                h[l] = R.gru_cell(inp, h[l], *w)
            else:
                h[l], c[l] = R.lstm_cell(inp, h[l], c[l], *w)
            inp = h[l] * damp if l == 0 else h[l]
        lg = inp @ params["linear.weight"].t() + params["linear.bias"]
        tv = torch.topk(lg, 2, dim=1)[0]
        gaps.append(tv[:, 0] - tv[:, 1]); scales.append(lg.abs().max(1)[0]); ids.append(lg.max(1)[1])
        tok = ids[-1] if tokens is None else tokens[:, t]
    return torch.stack(gaps, 1), torch.stack(scales, 1), torch.stack(ids, 1)


def _decoding_inputs():
    """(name, family, cell, params, feat) of everything the GPU file decodes from: the greedy cases of the plain decoders, those of
    the attention decoders (their own seed and scales on eight_long) and the beam inputs of both (END_BOOST on <end>, 3 images)"""
    for cell in CELLS:
        for case in Z.GREEDY_CASES:
            yield f"greedy {case}", "plain", cell, *Z.problem(case, cell, True)[:2]
        for case in Z.ATTN_GREEDY_CASES:
            yield f"greedy attention {case}", "attn", cell, *Z.attn_problem(case, cell, True)[:2]
        for family in ("plain", "attn"):
            params, feat = Z.beam_inputs(family, cell, True)
            yield f"beam {family}", family, cell, params, feat[:Z.BEAM_IMAGES]


def test_layer_zero_reaches_the_logits_of_the_decoding_cases():
    """what layer 0 computes must be visible seven layers up in everything the greedy and beam checks decode from"""
    for name, family, cell, params, feat in _decoding_inputs():
        walk = _greedy_gaps if family == "plain" else _attn_greedy_gaps
        p = {k: v.double().clone() for k, v in params.items()}
        if name.startswith("beam"):
            # the boost is a constant on one logit and says nothing about layer 0; with it the arg-max walk ends at once
            p["linear.bias"][2] -= Z.END_BOOST
        gap, scale, ids = walk(p, feat.double(), cell, 1.0)
        gap2, _, _ = walk(p, feat.double(), cell, 0.0, tokens=ids)
        rel = (gap2 - gap).abs() / scale
        moved = rel.median().item()
        print(f"MEASURE depth {name} {cell}: change of the top-two gap over 5 steps, median {moved:.2e} smallest {rel.min().item():.2e} "
              f"of max |logit|")
        assert moved >= DEPTH_GAP, (name, cell, moved)


# ---- seeded faults -------------------------------------------------------------------------------------------------------------

def _margin(case, cell, fault, dropout=False):
    """the largest (distance / bound) over the compared tensors and both norms, bf16 bounds on the bf16 inputs (the fp32 bound,
    2e-4 of the tensor's scale, is tighter than every one of them)"""
    ref = Z.grads(case, cell, True, None, False, dropout)
    got = Z.grads(case, cell, True, fault, False, dropout)
    worst = (0.0, None)
    for k, (l2, mx) in Z.distance(got[2], ref[2]).items():
        bl2, bmx = Z.bf16_bounds("dropout" if dropout else "plain", case, cell, k)
        worst = max(worst, (l2 / bl2, k), (mx / bmx, k), key=lambda v: v[0])
    return worst, abs(got[0] - ref[0])


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("case", list(Z.CASES))
@pytest.mark.parametrize("fault", Z.FAULTS)
def test_seeded_fault_is_caught_where_it_reaches_and_nowhere_else(fault, case, cell):
    (m, k), dloss = _margin(case, cell, fault)
    print(f"MEASURE fault {fault} {case} {cell}: {m:.2e} bounds ({k}), |d loss| {dloss:.2e}")
    if Z.reaches(fault, case):
        assert m >= FAULT_MARGIN, (fault, case, cell, m, k)
    else:
        assert m == 0.0 and dloss == 0.0, (fault, case, cell, m)


def test_fault_reach_is_as_the_cases_are_meant():
    reach = {f: [c for c in Z.CASES if Z.reaches(f, c)] for f in Z.FAULTS + Z.DROPOUT_FAULTS}
    assert reach["second_group_lost"] == ["seven_narrow", "eight_long", "eight_short", "eight_wide"]      # `six` fills one group exactly
    assert reach["cells_capped_at_5"] == ["eight_long"]
    assert reach["layer_reads_two_below"] == reach["carry_of_neighbour"] == ["seven_narrow", "eight_long", "eight_short", "eight_wide"]
    assert reach["late_diagonal_from_zero"] == ["six", "eight_long", "eight_short", "eight_wide"]     # seven_narrow: E != H
    assert "eight_long" in reach["mask_site_off_by_one"]


@pytest.mark.parametrize("cell", CELLS)
def test_mask_site_fault_is_caught_by_the_dropout_case(cell):
    (m, k), _ = _margin("eight_long", cell, "mask_site_off_by_one", True)
    print(f"MEASURE fault mask_site_off_by_one eight_long {cell}: {m:.2e} bounds ({k})")
    assert m >= FAULT_MARGIN, (cell, m, k)


# ---- bf16 storage floors -------------------------------------------------------------------------------------------------------

def _close(now, recorded):
    """a floor that fp32 arithmetic enters, recomputed here against its record: fp32 sums on another CPU may round a stored value the
    other way somewhere, so the match is held to a factor of 2, not to the digit (as tests/test_attention_geometry_inputs.py does)"""
    return recorded / 2 <= now <= recorded * 2


def _floors():
    out = {}
    for family, cases in (("plain", list(Z.CASES)), ("attn", list(Z.ATTN_CASES)), ("dropout", ["eight_long"])):
        for case in cases:
            for cell in CELLS:
                for k, (l2, mx) in Z.storage_distance(case, cell, family).items():
                    pl2, pmx = Z.project_bounds(family, k)
                    print(f"MEASURE floor {family} {case} {cell} {k}: rel_l2 {l2:.2e} rel_max {mx:.2e} (project bounds {pl2:.0e}, {pmx:.0e})")
                    if k == "attn.full_att.bias":      # analytically zero: held to the sum it cancels, not to a relative bound
                        continue
                    if l2 >= pl2 / 4 or mx >= pmx / 4:
                        out[(family, case, cell, k)] = (l2, mx)
    return out


def test_recorded_storage_floors_are_the_computed_ones():
    """Z.STORAGE_FLOORS holds exactly the gradients that bf16 storage alone moves by a quarter of the project's bound or more, with
    the distances computed here (float64 on both sides: to the three digits recorded)"""
    got = _floors()
    for key, v in sorted(got.items()):
        print(f"    {key!r}: ({v[0]:.2e}, {v[1]:.2e}),")
    assert sorted(got) == sorted(Z.STORAGE_FLOORS), (sorted(set(got) ^ set(Z.STORAGE_FLOORS)))
    for key, (l2, mx) in got.items():
        rl2, rmx = Z.STORAGE_FLOORS[key]
        assert abs(l2 - rl2) <= 0.006 * rl2 and abs(mx - rmx) <= 0.006 * rmx, (key, (l2, mx), (rl2, rmx))


def test_recorded_logp_floors_and_greedy_gap_are_the_computed_ones():
    got = {}
    for family, cases in (("plain", Z.LOGP_CASES), ("attn", Z.LOGP_CASES)):
        for case in cases:
            for cell in CELLS:
                l2, mx = Z.logp_distance(Z.oracle_logp(family, case, cell, True, True), Z.oracle_logp(family, case, cell, True))
                print(f"MEASURE floor token_logp {family} {case} {cell}: rel_l2 {l2:.2e} rel_max {mx:.2e}")
                if l2 >= Z.GRAD_L2 / 4 or mx >= Z.GRAD_MAX / 4:
                    got[(family, case, cell)] = (l2, mx)
    print("LOGP_FLOORS", {k: (float(f"{a:.2e}"), float(f"{b:.2e}")) for k, (a, b) in got.items()})
    assert sorted(got) == sorted(Z.LOGP_FLOORS)
    for key, (l2, mx) in got.items():
        rl2, rmx = Z.LOGP_FLOORS[key]
        assert abs(l2 - rl2) <= 0.006 * rl2 and abs(mx - rmx) <= 0.006 * rmx, (key, (l2, mx), (rl2, rmx))
    gaps = {}
    for cell in CELLS:
        for bf16 in (False, True):
            floor = max(Z.attn_greedy_floor(case, cell, bf16) for case in Z.ATTN_GREEDY_CASES)
            gaps[(cell, bf16)] = float(f"{floor:.2e}")
            print(f"MEASURE floor attention greedy {cell} {'bf16' if bf16 else 'fp32'}: |d logp| {floor:.3e}")
    print("ATTN_GAP", {k: f"4 * {v:.2e}" for k, v in gaps.items()})
    assert sorted(gaps) == sorted(Z.ATTN_GAP)
    for k, v in gaps.items():
        assert _close(4 * v, Z.ATTN_GAP[k]), (k, v, Z.ATTN_GAP[k])


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cell", CELLS)
def test_attention_greedy_walk_leaves_few_steps_within_the_gap(cell, bf16):
    """the GPU test compares a token only where the oracle's top-two gap exceeds ATTN_GAP and allows 0.10 of the steps to fall
    within it: the float64 oracle's own walk must leave room"""
    from tests import _attention_geometry_cases as G
    steps = within = 0
    for case in Z.ATTN_GREEDY_CASES:
        params, feat, _, _ = Z.attn_problem(case, cell, bf16)
        gap = G.top_two_gap(G.greedy_walk(params, feat, cell, bf16)[0])
        steps += gap.numel(); within += int((gap <= Z.ATTN_GAP[(cell, bf16)]).sum())
    print(f"MEASURE attention greedy {cell} {'bf16' if bf16 else 'fp32'}: {within} of {steps} steps within the gap ({within / steps:.3f})")
    assert within / steps <= 0.09


def test_bf16_greedy_restatement_in_fp32_arithmetic_against_the_greedy_bounds():
    """The GPU test holds the bf16 greedy ids to DELTA and AGREE of tests/test_gpu_decoder_bench_shape.py.  No fp32 implementation
    is owed more than the storage restatement computed in fp32 instead of float64 gives.  six and eight_long: it agrees with its
    float64 self on every row.  eight_wide (eight layers of 512 units, 777 words, 25 steps) amplifies a bf16 rounding of h that an
    fp32 sum decides differently: measured here over six orders of summation of the same model (hidden units permuted), the GRU keeps
    29 to 32 of 33 rows with gaps up to 8.0e-3 of max |logit|, the LSTM 19 to 25 rows with gaps of 9.9e-3 to 3.1e-2; scales from 2 to
    5, vocabulary scales from 6 to 40 and seven seeds gave no inputs at which every order keeps 30 rows.  The GPU test therefore gives
    the eight_wide LSTM the share tests/test_gpu_decoder_bench_shape.py gives its own sensitive LSTM stack (2/3) and keeps DELTA; this
    test fails if that premise goes away."""
    from tests.test_gpu_decoder_bench_shape import AGREE, DELTA
    for case in Z.GREEDY_CASES:
        for cell in CELLS:
            share, gap = Z.plain_greedy_floor(case, cell)
            print(f"MEASURE floor plain greedy {case} {cell}: fp32 against float64 arithmetic agree on {share:.3f} of the rows, worst gap {gap:.2e}")
            if case != "eight_wide":
                assert share >= AGREE and gap <= DELTA, (case, cell, share, gap)
            elif cell == "lstm":
                assert share < AGREE, "the fp32 restatement keeps AGREE of the rows: the eight_wide LSTM needs no share of its own"


def test_recorded_beam_floors_are_the_computed_ones():
    got = {}
    for family in ("plain", "attn"):
        for cell in CELLS:
            for bf16 in (False, True):
                f = Z.beam_floor(family, cell, bf16)
                print(f"MEASURE floor beam {family} {cell} {'bf16' if bf16 else 'fp32'}: {f}")
                got[(family, cell, bf16)] = tuple(float(f"{f[k]:.2e}") for k in ("nll_word", "nll", "a_max", "a_l2"))
                # the three images the GPU searches: some hypotheses end within 8 words, and not every one at once
                assert f["harvested"] > 0, (family, cell, bf16)
    for k, v in got.items():
        print(f"    {k!r}: {v!r},")
    assert sorted(got) == sorted(Z.BEAM_FLOORS)
    for k, v in got.items():
        assert all(_close(a, b) for a, b in zip(v, Z.BEAM_FLOORS[k])), (k, v, Z.BEAM_FLOORS[k])


def test_recorded_sample_floors_are_the_computed_ones():
    got = {}
    for family in ("plain", "attn"):
        for cell in CELLS:
            for bf16 in (False, True):
                got[(family, cell, bf16)] = tuple(float(f"{v:.2e}") for v in Z.sample_floor(family, cell, bf16))
    for k, v in got.items():
        print(f"    {k!r}: {v!r},")
    assert sorted(got) == sorted(Z.SAMPLE_FLOORS)
    for k, v in got.items():
        assert all(_close(a, b) for a, b in zip(v, Z.SAMPLE_FLOORS[k])), (k, v, Z.SAMPLE_FLOORS[k])


def test_recorded_scheduled_sampling_floors_are_the_computed_ones():
    got = {}
    for family in ("plain", "attn"):
        for cell in CELLS:
            for bf16 in (False, True):
                got[(family, cell, bf16)] = float(f"{Z.sched_floor(family, cell, bf16):.2e}")
    for k, v in got.items():
        print(f"    {k!r}: {v:.2e},")
    assert sorted(got) == sorted(Z.SCHED_FLOORS)
    for k, v in got.items():
        assert _close(v, Z.SCHED_FLOORS[k]), (k, v, Z.SCHED_FLOORS[k])
    # the roll-in replaces about half of the valid slots, and the oracle's own mixed ids differ from the caption there
    from tests import _scheduled_sampling_cases as K
    ids, rep, _ = Z.sched_roll_in("plain", "gru", True, Z.sched_uniforms())
    cap, lens = Z.problem(Z.SCHED_CASE, "gru", True)[2:]
    valid = int(K.valid_slots("rnn", lens, cap.shape[1]).sum())
    assert 0.35 * valid < int(rep.sum()) < 0.65 * valid and int((ids != cap).sum()) > 0.25 * valid


# ---- limits --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [0, 9])
def test_num_layers_outside_1_to_8_is_refused_by_every_class(L):
    from showtell_amd.rnn import RNN
    from showtell_amd.rnn_attn import RNN_Attn
    from showtell_amd.rnn_attn_LSTM import RNN_Attn as RNN_Attn_LSTM
    from showtell_amd.rnn_lstm import RNN as RNN_LSTM
    for cls in (RNN, RNN_LSTM):
        with pytest.raises(ValueError):
            cls(16, 16, Z.V, L)
    for cls in (RNN_Attn, RNN_Attn_LSTM):
        with pytest.raises(ValueError):
            cls(16, Z.ATTN["F"], Z.ATTN["A"], 16, Z.V, L)
    RNN(16, 16, Z.V, Z.MAX_LAYERS), RNN_Attn_LSTM(16, Z.ATTN["F"], Z.ATTN["A"], 16, Z.V, Z.MAX_LAYERS)     # 8 is legal


@pytest.mark.parametrize("L", [0, 9])
def test_planners_and_entry_points_refuse_the_layer_count_before_any_launch(L):
    """host-only (it loads the built library, as tests/test_decoder_workspace.py does, and fails where that has not been built):
    every st_*_workspace_bytes planner of the decoders answers 0 for a hand-built descriptor with L = 0 or 9, and
    st_rnn_forward returns its error at the layer check, before it reads a pointer"""
    import ctypes as C

    from showtell_amd import ShowTellHipError, _lib
    from showtell_amd._lib import check, lib
    from tests.test_decoder_workspace import _rnn_params, _seq
    s = _seq([3, 2])
    for cell in CELLS:
        for dtype in ("f32", "bf16"):
            p = _rnn_params(cell, dtype, 16, 16, 16, L, Z.V)
            a = _lib.AttnParams()
            a.rnn = _rnn_params(cell, dtype, 16, 32, 16, L, Z.V)
            a.F, a.A, a.P = Z.ATTN["F"], Z.ATTN["A"], Z.ATTN["P"]
            got = dict(rnn=lib().st_rnn_workspace_bytes(C.byref(p), C.byref(s)), greedy=lib().st_rnn_greedy_workspace_bytes(C.byref(p), 2),
                       sample=lib().st_rnn_sample_workspace_bytes(C.byref(p), 2), attn=lib().st_attn_workspace_bytes(C.byref(a), C.byref(s)),
                       attn_greedy=lib().st_attn_greedy_workspace_bytes(C.byref(a), 2),
                       attn_sample=lib().st_attn_sample_workspace_bytes(C.byref(a), 2),
                       attn_beam=lib().st_attn_beam_workspace_bytes(C.byref(a), 2, 4, 14, None, None))
            assert all(v == 0 for v in got.values()), (cell, dtype, got)
            with pytest.raises(ShowTellHipError, match=f"num_layers={L} out of range"):
                check(lib().st_rnn_forward(C.byref(p), C.byref(s), None, None, 0, None, 0, 0, None, 0, None, None, None), "st_rnn_forward")
    # and 8 layers are planned
    p = _rnn_params("gru", "f32", 16, 16, 16, Z.MAX_LAYERS, Z.V)
    assert lib().st_rnn_workspace_bytes(C.byref(p), C.byref(s)) > 0 and lib().st_rnn_greedy_workspace_bytes(C.byref(p), 2) > 0


@pytest.mark.parametrize("cell", CELLS)
def test_greedy_planner_reserves_no_pipeline_bytes_at_eight_layers(cell, monkeypatch):
    """eight_wide is the pipelined decoder's shape (bf16, E = H = 512) at a depth it must decline: the greedy workspace carries its
    buffers at 5 layers and not at 6, 7 or 8, where the count is that of the launch chain's own buffers (Z.greedy_chain_bytes, a
    mirror of make_greedy_plan without the pipeline's region) to the byte; the counts do not depend on ST_DECODE_PIPE"""
    import ctypes as C

    from showtell_amd._lib import lib
    from tests.test_decoder_workspace import _rnn_params
    c = Z.CASES["eight_wide"]
    B = len(c["lens"])

    def nbytes(dtype, L):
        p = _rnn_params(cell, dtype, c["E"], c["E"], c["H"], L, c["V"])
        return lib().st_rnn_greedy_workspace_bytes(C.byref(p), B)
    monkeypatch.delenv("ST_DECODE_PIPE", raising=False)
    for pipe in (None, "0"):
        if pipe is not None:
            monkeypatch.setenv("ST_DECODE_PIPE", pipe)
        for L in (6, 7, c["L"]):                       # the launch chain's buffers to the byte: nothing of the pipeline's behind them
            assert nbytes("bf16", L) == Z.greedy_chain_bytes(cell, True, c["E"], c["H"], L, c["V"], B), L
            assert nbytes("f32", L) == Z.greedy_chain_bytes(cell, False, c["E"], c["H"], L, c["V"], B), L
        assert nbytes("bf16", 5) > Z.greedy_chain_bytes(cell, True, c["E"], c["H"], 5, c["V"], B)      # five layers carry them
        assert nbytes("f32", 5) == Z.greedy_chain_bytes(cell, False, c["E"], c["H"], 5, c["V"], B)
