"""The implicit GEMM (csrc/igemm.hip: st_conv, st_conv_batch) through the C ABI with hand-built descriptors, element by element
against the float64 oracle of tests/_igemm_cases.py under the bounds derived there (tests/test_igemm_inputs.py shows that the
oracle's own float32 / bf16 replica keeps them and that every seeded fault breaks them).  Every case first asserts that
st_conv_last_route() reports the route the case table names -- tile, wave count, K chunking, MODE and main loop -- so that a case
cannot drift onto another kernel unnoticed.  Checked on every case: each canary of y (pad columns, the guard row after row M - 1,
the 16 bytes in front of an offset base) is unchanged, no NaN of a pad column of x / w / the residual reached the result, and two
runs are bit-equal wherever no atomics are involved.  Largest measured error / bound on an MI355X: DESIGN.md section 7, row
'implicit GEMM'; the MEASURE lines print it per case."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import _igemm_cases as G

pytestmark = pytest.mark.gpu

ENV_KNOBS = sorted(k for k in os.environ if k.startswith("ST_IGEMM_"))


def _lib():
    from showtell_amd import _lib
    return _lib


def _route():
    out = (C.c_int * 8)()
    n = _lib().lib().st_conv_last_route(out)
    return tuple(out), n


def _dev(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(G.TORCH_DTYPE[dtype]).cuda()


def _problem(name, dtype, member=0, changes=None):
    """Device buffers and the st_conv_desc of one member; `changes` overrides descriptor fields (the refusal cases)."""
    L = _lib()
    s = G.CASES[name]
    p = G.inputs(name, dtype, member)
    odt = G.out_dtype(s, dtype)
    t = dict(x=_dev(p["x"], dtype), w=_dev(p["w"], dtype), ybuf=_dev(p["y0"], odt), residual=_dev(p["residual"], odt))
    for k in ("bias", "scale", "shift", "in_stats", "in_gamma", "in_beta"):
        t[k] = _dev(p.get(k), "float32")
    t["stats"] = _dev(p["stats0"], "float32")
    d = dict(G.descriptor(s, dtype), **(changes or {}))
    desc = L.ConvDesc()
    for k, _ in L.ConvDesc._fields_:
        if k == "y":
            setattr(desc, k, t["ybuf"].data_ptr() + p["lead"] * t["ybuf"].element_size() if d["y"] else None)
        elif k in ("x", "w", "bias", "scale", "shift", "residual", "stats", "in_stats", "in_gamma", "in_beta"):
            setattr(desc, k, None if not d[k] else (t[k] if t[k] is not None else t["x"]).data_ptr())
        else:
            setattr(desc, k, d[k])
    return t, desc, p


def _read(s, dtype, t, p):
    """(result [M][N], canaries, statistics) of a finished launch as float64, plus the raw bytes of y for bit comparisons."""
    torch.cuda.synchronize()
    ybuf = t["ybuf"].cpu()
    res, can = G.split_y(s, dtype, ybuf.double().numpy(), p["lead"])
    stats = None if t["stats"] is None else t["stats"].cpu().double().numpy()
    return res, can, stats, ybuf.view(torch.uint8).numpy().copy()


def _check(what, s, dtype, p, ref, res, can, stats):
    _, can0 = G.split_y(s, dtype, p["y0"], p["lead"])
    assert np.array_equal(can, can0), f"{what}: {(can != can0).sum()} canaries of y were written"
    assert np.isfinite(res).all(), f"{what}: {(~np.isfinite(res)).sum()} results are not finite: a pad column was read"
    r = G.ratios(res, stats, ref)
    print(f"MEASURE {what}: " + " ".join(f"{k} error / bound {v:.3f}" for k, v in r.items()))
    assert max(r.values()) < 1.0, (what, r)


class _Tuned:
    """st_tune(ring, kc, w8) for the duration of a case, the defaults afterwards."""

    def __init__(self, knobs):
        self.knobs = knobs

    def __enter__(self):
        _lib().lib().st_tune(*self.knobs)

    def __exit__(self, *exc):
        _lib().lib().st_tune(*G.KNOBS)


def _run_single(name, dtype, member=0):
    L = _lib()
    s = G.CASES[name]
    t, desc, p = _problem(name, dtype, member)
    _, n0 = _route()
    rc = L.lib().st_conv(C.byref(desc), L.stream())
    assert rc == 0, L.lib().st_last_error().decode()
    got, n1 = _route()
    assert n1 == n0 + 1, "one igemm launch per st_conv call"
    return got, _read(s, dtype, t, p), p


@pytest.mark.parametrize("name,dtype", [(n, dt) for n, dt in G.RUNS if G.CASES[n]["group"] == 1 and not n.startswith("grp")])
def test_st_conv_takes_its_route_and_matches_the_float64_oracle(name, dtype):
    s = G.CASES[name]
    if s["knobs"] != G.KNOBS and ENV_KNOBS:
        pytest.skip(f"{', '.join(ENV_KNOBS)} set in the environment: the knob-only routes are not the ones st_tune would give")
    with _Tuned(s["knobs"]):
        got, (res, can, stats, raw), p = _run_single(name, dtype)
        want = G.route(s, dtype)
        assert got == want == G.table_route(s, dtype), dict(zip(G.ROUTE_FIELDS, zip(got, want)))
        _check(f"{dtype} {name}", s, dtype, p, G.oracle(name, dtype), res, can, stats)
        if not s["stats"] and not s["split_k"]:       # no atomics: the same bits every time
            _, (_, _, _, raw2), _ = _run_single(name, dtype)
            assert np.array_equal(raw, raw2), f"{(raw != raw2).sum()} bytes of y differ between two runs"


@pytest.mark.parametrize("dtype", G.DTYPES)
@pytest.mark.parametrize("name", ["grp1", "grp12"])
def test_a_grouped_launch_equals_single_launches_bit_for_bit(name, dtype):
    L = _lib()
    s = G.CASES[name]
    n = s["group"]
    with _Tuned(s["knobs"]):
        probs = [_problem(name, dtype, i) for i in range(n)]
        assert len({t[k].data_ptr() for t, _, _ in probs for k in ("x", "w", "ybuf", "bias")}) == 4 * n      # distinct pointers
        arr = (L.ConvDesc * n)(*[d for _, d, _ in probs])
        _, n0 = _route()
        assert L.lib().st_conv_batch(arr, n, L.stream()) == 0, L.lib().st_last_error().decode()
        got, n1 = _route()
        assert n1 == n0 + 1 and got == G.route(s, dtype) == G.table_route(s, dtype), got
        assert got[6] == n
        for i, (t, _, p) in enumerate(probs):
            res, can, stats, raw = _read(s, dtype, t, p)
            _check(f"{dtype} {name} member {i}", s, dtype, p, G.oracle(name, dtype, i), res, can, stats)
            route1, (_, _, _, raw1), _ = _run_single(name, dtype, i)
            assert route1[:6] == got[:6] and route1[6] == 1
            assert np.array_equal(raw, raw1), f"member {i}: {(raw != raw1).sum()} bytes differ from the single launch"


SENTINEL_BYTES = 1 << 22


@pytest.mark.parametrize("dtype", G.DTYPES)
def test_refusals_return_an_error_launch_nothing_and_leave_y_and_the_route_alone(dtype):
    L = _lib()
    lib = L.lib()
    err = lambda: lib.st_last_error().decode()
    with _Tuned(G.KNOBS):
        # a launch first, so that there is a record to leave alone; the accepted bases are one change away from every refusal
        for base in ("refusal_base", "refusal_k72"):
            got, (res, can, stats, _), p = _run_single(base, dtype)
            _check(f"{dtype} {base}", G.CASES[base], dtype, p, G.oracle(base, dtype), res, can, stats)
        before = _route()
        spare = torch.zeros(SENTINEL_BYTES // 4, device="cuda")          # stands in for the optional pointers a change switches on

        def problem(base, changes):
            t, desc, p = _problem("refusal_" + base, dtype, changes=changes)
            for k in ("bias", "scale", "shift", "residual", "stats", "in_stats", "in_gamma", "in_beta"):
                if dict(G.refusal_descriptor(base, changes, dtype))[k]:
                    setattr(desc, k, spare.data_ptr())
            return t, desc, p

        def untouched(t, p, what):
            torch.cuda.synchronize()
            assert np.array_equal(t["ybuf"].cpu().double().numpy(), p["y0"]), f"{what}: y was written"
            assert _route() == before, f"{what}: the route record changed"

        for label, base, changes, msg in G.REFUSALS:
            t, desc, p = problem(base, changes)
            assert lib.st_conv(C.byref(desc), L.stream()) != 0, label
            assert msg in err(), (label, err())
            untouched(t, p, label)
        assert lib.st_conv(None, L.stream()) != 0 and "null pointer" in err()
        for label, n, changes, msg in G.BATCH_REFUSALS:
            t0, d0, p0 = problem("base", {})
            t1, d1, p1 = problem("base", changes)
            arr = (L.ConvDesc * 13)(*([d0, d1] + [d0] * 11))
            assert lib.st_conv_batch(arr, n, L.stream()) != 0, label
            assert msg in err(), (label, err())
            untouched(t0, p0, label); untouched(t1, p1, label)
        assert lib.st_conv_batch(None, 1, L.stream()) != 0 and "problems per launch" in err()
        assert _route() == before and (spare == 0).all().item()
