"""tests/_igemm_cases.py checked on the CPU: every case takes the route the table names for it, the float64 oracle is the
convolution torch computes, the oracle's own float32 / bf16 replica stays inside every bound, every seeded fault leaves one, and
the descriptors the GPU file passes are ones fill_args accepts (the refusal cases violate exactly one requirement)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _igemm_cases as G

RUNS = G.RUNS
BIG = 4e6       # M * N * K above which the fma-chain replica runs on the corner and middle rows / columns only


def _subset(name):
    g = G.geometry(G.CASES[name])
    M, N = g["M"], g["N"]
    if M * N * g["K"] <= BIG:
        return None, None
    return sorted({0, 1, 63, 64, M // 2, M - 2, M - 1}), sorted({0, 1, N // 2, N - 5, N - 4, N - 3, N - 2, N - 1})


@pytest.mark.parametrize("name,dtype", RUNS)
def test_every_case_takes_the_route_the_table_names(name, dtype):
    s = G.CASES[name]
    assert G.route(s, dtype) == G.table_route(s, dtype), s["why"]


def test_the_table_reaches_every_route_of_the_dispatch():
    routes = {G.route(G.CASES[n], dt)[:6] for n, dt in RUNS}
    default = {G.route(G.CASES[n], dt)[:6] for n, dt in RUNS if G.CASES[n]["knobs"] == G.KNOBS}
    assert (2, 128, 128, 4, 4, 1) in default                                                # the three-buffer route on its own conditions
    for tile in ((128, 64, 8), (64, 128, 4), (128, 128, 8)):
        assert {(0,) + tile + (8, m) for m in (0, 1)} <= default, tile
    assert {(0, 128, 64, 4, 4, 1), (0, 128, 128, 8, 4, 1), (0, 64, 128, 4, 4, 1)} <= default     # KC 4 on each tile
    assert {r[5] for r in default} == {0, 1, 2}
    assert {(0, 128, 128, 4, 8, 0), (0, 128, 64, 4, 8, 0), (0, 256, 128, 8, 8, 0), (0, 256, 128, 8, 8, 1)} <= routes - default
    # the thresholds themselves: a tile row or two fewer and the case would be somewhere else
    t64 = G.CASES["g_t64"]
    assert G.route(dict(t64, B=t64["B"] - 64), "float32")[1:3] == (128, 128)        # 17 x 15 = 255 tiles of 64 rows
    t128 = G.CASES["g_t128"]
    assert G.route(dict(t128, B=2816), "float32")[1:3] == (64, 128)                 # 22 x 17 = 374 tiles of 128 rows
    assert G.route(dict(G.CASES["kc4_128"], B=4095), "float32")[4] == 8
    assert G.route(dict(G.CASES["three_buffer"], B=1920), "bfloat16")[0] == 0


@pytest.mark.parametrize("name,dtype", [(n, dt) for n, dt in RUNS if G.CASES[n]["KH"] * G.CASES[n]["KW"] > 1 and not G.CASES[n]["xf"]])
def test_the_oracle_is_the_convolution_torch_computes(name, dtype):
    s, g, p = G.CASES[name], G.geometry(G.CASES[name]), G.inputs(name, dtype)
    got = G.oracle(name, dtype)["y"].reshape(s["B"], g["Ho"], g["Wo"], s["N"])
    w = torch.from_numpy(p["wl"].reshape(s["N"], s["KH"], s["KW"], s["Cin"])).permute(0, 3, 1, 2)
    if g["sliding"]:      # Cin / ldx neighbouring pixels of a row are one tap: a KH x (Cin / ldx) filter over ldx channels
        kw = s["Cin"] // g["ldx"]
        x = torch.from_numpy(p["x"].reshape(s["B"], s["Hin"], s["Win"], g["ldx"])).permute(0, 3, 1, 2)
        w = torch.from_numpy(p["wl"].reshape(s["N"], s["KH"], kw, g["ldx"])).permute(0, 3, 1, 2)
        ref = F.conv2d(x, w, None, s["stride"], 0)
    else:
        x = torch.from_numpy(p["x"].reshape(s["B"], s["Hin"], s["Win"], g["ldx"])[..., :s["Cin"]]).permute(0, 3, 1, 2)
        ref = F.conv2d(x, w, None, s["stride"], s["pad"])
    ref = ref.permute(0, 2, 3, 1).numpy()
    assert ref.shape == got.shape
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("name,dtype", RUNS)
def test_the_replica_stays_inside_every_bound(name, dtype):
    rows, cols = _subset(name)
    ref = G.oracle(name, dtype, rows=rows, cols=cols)
    y, stats = G.replica(name, dtype, rows=rows, cols=cols)
    r = G.ratios(y, stats, ref)
    assert set(r) == ({"y", "sum", "sumsq"} if stats is not None else {"y"})
    assert max(r.values()) < 1.0, r
    assert (ref["bound"] > 0).all() and np.isfinite(ref["y"]).all()       # no pad column reached the oracle


@pytest.mark.parametrize("fault", G.FAULTS)
def test_every_seeded_fault_leaves_a_bound(fault):
    runs = [(n, dt) for n, dt in RUNS if G.fault_applies(fault, G.CASES[n], dt)]
    assert runs, f"no case for {fault}"
    for name, dtype in runs:
        ref, bad = G.oracle(name, dtype), G.oracle(name, dtype, fault=fault)
        r = G.ratios(bad["y"], bad["stats"], ref)
        assert max(r.values()) > 1.0, (name, dtype, r)


def test_the_faults_that_need_a_pad_a_tail_or_a_replica_have_cases_of_every_kind():
    kinds = {f: {(G.route(G.CASES[n], dt)[1:3]) for n, dt in RUNS if G.fault_applies(f, G.CASES[n], dt)} for f in G.FAULTS}
    assert {(128, 64), (128, 128)} <= kinds["pad_neighbour"] and {(128, 64), (128, 128)} <= kinds["xf_pad_relu_shift"]
    assert {(128, 64), (64, 128), (128, 128)} <= kinds["drop_tail_channels"]
    assert {(128, 64), (128, 128)} <= kinds["replica0_only"]
    assert kinds["stats_after_rounding"] and kinds["bias_per_slice"] and kinds["korder_misread"] and kinds["ldx_as_cin"]


@pytest.mark.parametrize("name,dtype", RUNS)
def test_inputs_are_asymmetric_padded_and_of_their_storage_type(name, dtype):
    s, g, p = G.CASES[name], G.geometry(G.CASES[name]), G.inputs(name, dtype)
    dt = G.TORCH_DTYPE[dtype]
    for k in ("x", "w"):
        a = torch.from_numpy(p[k])
        assert torch.equal(a.to(dt).double().nan_to_num(7.0), a.nan_to_num(7.0)), k      # exactly representable
    x = p["x"].reshape(-1, g["ldx"])
    assert np.isnan(x[:, s["Cin"]:]).all() and np.isnan(p["w"][:, g["K"]:]).all()
    assert np.isfinite(x[:, :s["Cin"]]).all() and np.isfinite(p["w"][:, :g["K"]]).all()
    wl = p["wl"]
    head = lambda a: a[:512, :512]
    for a in (head(wl), head(wl).T, head(x[:, :min(s["Cin"], g["ldx"])])):      # no two rows, no two columns alike
        if a.shape[1] >= 8:
            assert len(np.unique(a, axis=0)) == len(a)
    if wl.shape[0] == wl.shape[1]:
        assert not np.array_equal(wl, wl.T)
    if p["residual"] is not None:
        assert np.isnan(p["residual"][:, s["N"]:]).all()
    res, can = G.split_y(s, dtype, p["y0"], p["lead"])
    assert (can <= -100).all() and len(can) == p["lead"] + g["M"] * s["ldy_pad"] + g["ldy"]
    assert s["accumulate"] or (res <= -100).all()
    odt = G.TORCH_DTYPE[G.out_dtype(s, dtype)]
    assert torch.equal(torch.from_numpy(p["y0"]).to(odt).double(), torch.from_numpy(p["y0"]))
    assert G.inputs(name, dtype) is p                                             # computed once, shared


@pytest.mark.parametrize("name,dtype", RUNS)
def test_the_descriptors_are_ones_fill_args_accepts(name, dtype):
    assert G.desc_errors(G.descriptor(G.CASES[name], dtype)) == []


@pytest.mark.parametrize("dtype", G.DTYPES)
def test_every_refusal_violates_exactly_one_requirement(dtype):
    for base in ("base", "k72"):
        assert G.desc_errors(G.refusal_descriptor(base, {}, dtype)) == []
    for label, base, changes, msg in G.REFUSALS:
        errs = G.desc_errors(G.refusal_descriptor(base, changes, dtype))
        assert len(errs) == 1, (label, errs)
    for label, n, changes, msg in G.BATCH_REFUSALS:
        if changes:
            assert len(G.desc_errors(G.refusal_descriptor("base", changes, dtype))) <= 1, label
    assert len({r[0] for r in G.REFUSALS}) == len(G.REFUSALS)
