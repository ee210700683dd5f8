"""The encoder head (head.linear_bn1d: st_linear_bn1d_forward / _backward, csrc/head_optim.hip) against the float64 oracle of
tests/_head_cases.py over batch sizes, widths and GEMM routes, under the bounds that tests/test_head_inputs.py derives from the
oracle's own float32 replica and shows to have power.  Largest measured error / bound on an MI355X: DESIGN.md section 7 (row
'encoder head')."""
import pytest
import torch
from torch import nn

from tests import _head_cases as H

pytestmark = pytest.mark.gpu

TORCH_DTYPE = {"float32": torch.float32, "bfloat16": torch.bfloat16}
# the route each case exists to reach: split-K in (fp32, bf16)
ROUTES = {"tiny": (False, False), "odd": (False, False), "single": (True, True), "split_edge": (True, True), "long_k": (False, False),
          "tall": (True, False)}
RUNS = [(c, m) for c, v in H.CASES.items() for m in v[3]]


def _modules(p, train):
    """nn.Linear and nn.BatchNorm1d on the GPU from the case's tensors, every .grad at the non-zero start g0."""
    E, F = p["W"].shape
    lin, bn = nn.Linear(F, E), nn.BatchNorm1d(E, momentum=H.MOMENTUM, eps=H.EPS)
    lin.weight.data.copy_(p["W"]); lin.bias.data.copy_(p["b"])
    bn.weight.data.copy_(p["gamma"]); bn.bias.data.copy_(p["beta"])
    bn.running_mean.copy_(p["running_mean"]); bn.running_var.copy_(p["running_var"])
    lin, bn = lin.cuda().train(train), bn.cuda().train(train)
    for q, k in zip((lin.weight, lin.bias, bn.weight, bn.bias), H.GRADS):
        q.grad = p["g0_" + k].clone().cuda()
    return lin, bn


def _call(lin, bn, x, dy, train, dtype):
    from showtell_amd.head import linear_bn1d
    y = linear_bn1d(x, lin, bn, train, TORCH_DTYPE[dtype])
    (y * dy.cuda()).sum().backward()
    return y


def _got(p, lin, bn, y):
    out = {"y": y, "running_mean": bn.running_mean, "running_var": bn.running_var}
    for q, k in zip((lin.weight, lin.bias, bn.weight, bn.bias), H.GRADS):
        out[k] = q.grad.detach().cpu() - p["g0_" + k]                  # fp32, as the replica subtracts it
    return {k: v.detach().cpu() for k, v in out.items()}


def _compare(what, got, ref, train, dtype):
    errs, b = H.errors(got, ref, train), H.bounds(dtype)
    assert set(errs) == set(H.TENSORS)
    print(f"MEASURE {what}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    print(f"MEASURE {what}: worst error / bound = {max(errs[k] / b[k] for k in errs):.3f}")
    assert not H.outside(errs, dtype), {k: (errs[k], b[k]) for k in H.outside(errs, dtype)}


@pytest.mark.parametrize("dtype", H.DTYPES)
@pytest.mark.parametrize("case,mode", RUNS)
def test_forward_and_backward_match_the_float64_oracle(case, mode, dtype):
    B, F, E, _ = H.CASES[case]
    train = mode == "train"
    assert H.split_k(B, F, E, dtype) == ROUTES[case][H.DTYPES.index(dtype)]      # the route this case is here for
    p = H.inputs(case, dtype)
    lin, bn = _modules(p, train)
    y = _call(lin, bn, p["x"].cuda(), p["dy"], train, dtype)                    # fp32 x: cast by the head in bf16 mode
    assert y.shape == (B, E) and y.dtype == torch.float32
    assert int(bn.num_batches_tracked) == (1 if train else 0)
    _compare(f"{dtype} {case} {mode}", _got(p, lin, bn, y), H.run(case, dtype, train), train, dtype)


@pytest.mark.parametrize("dtype", H.DTYPES)
@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("case", H.ACCUMULATION_CASES)
def test_a_second_backward_accumulates(case, mode, dtype):
    """No zeroing in between: the gradients are g0 plus both calls', the running statistics those after two updates."""
    train = mode == "train"
    p = H.inputs(case, dtype)
    lin, bn = _modules(p, train)
    _call(lin, bn, p["x"].cuda(), p["dy"], train, dtype)
    y = _call(lin, bn, p["x2"].cuda(), p["dy2"], train, dtype)
    assert int(bn.num_batches_tracked) == (2 if train else 0)
    _compare(f"{dtype} {case} {mode} two calls", _got(p, lin, bn, y), H.run(case, dtype, train, steps=2), train, dtype)


@pytest.mark.parametrize("dtype", H.DTYPES)
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_a_strided_input_equals_the_dense_one_bit_for_bit(mode, dtype):
    """x as a column slice of a wider tensor that already has the compute dtype: the head must not read it as dense rows."""
    train = mode == "train"
    p = H.inputs("odd", dtype)
    B, F = p["x"].shape
    dt = TORCH_DTYPE[dtype]
    wide = torch.full((B, F + 24), 7.0, dtype=dt).cuda()
    wide[:, 8:8 + F] = p["x"].to(dt).cuda()
    view = wide[:, 8:8 + F]
    assert not view.is_contiguous() and view.dtype == dt
    res = []
    for x in (view.contiguous(), view):
        lin, bn = _modules(p, train)
        y = _call(lin, bn, x, p["dy"], train, dtype)
        res.append([y.detach(), bn.running_mean, bn.running_var, lin.weight.grad, lin.bias.grad, bn.weight.grad, bn.bias.grad])
    names = ["y", "running_mean", "running_var", "dW", "dbias", "dgamma", "dbeta"]
    for k, a, b in zip(names, *res):      # dbias too: B = 13 is one transpose tile, so one float atomic per column onto g0
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{k} differs in {(a != b).sum().item()} elements"
    _compare(f"{dtype} odd {mode} strided", _got(p, lin, bn, y), H.run("odd", dtype, train), train, dtype)


@pytest.mark.parametrize("dtype", H.DTYPES)
def test_workspace_size_is_the_three_aligned_regions(dtype):
    from showtell_amd._lib import dtype_code, lib
    for case, (B, F, E, _) in H.CASES.items():
        es = 2 if dtype == "bfloat16" else 4
        want = H.al256(B * H.up8(E) * es) + H.al256(E * H.up8(B) * es) + H.al256(F * H.up8(B) * es)
        assert lib().st_head_workspace_bytes(B, F, E, dtype_code(TORCH_DTYPE[dtype])) == want == H.workspace_bytes(B, F, E, dtype), case


SENTINEL = -123.25


def _raw(B, F, E, dtype):
    """Buffers for a direct call of the C entry points, large enough for the shape even if the call were not refused."""
    dt = TORCH_DTYPE[dtype]
    g = torch.Generator().manual_seed(5)
    t = {"x": torch.randn(B, F, generator=g).to(dt), "w": torch.randn(E, F, generator=g).to(dt), "bias": torch.zeros(E), "gamma": torch.ones(E),
         "beta": torch.zeros(E), "rm": torch.zeros(E), "rv": torch.ones(E), "z": torch.full((B, E), SENTINEL), "mean": torch.zeros(E), "rstd": torch.ones(E),
         "y": torch.full((B, E), SENTINEL), "dy": torch.randn(B, E, generator=g), "dw": torch.full((E, F), SENTINEL), "db": torch.full((E,), SENTINEL),
         "dg": torch.full((E,), SENTINEL), "dbeta": torch.full((E,), SENTINEL)}
    return {k: v.cuda() for k, v in t.items()}


def _forward(t, B, F, E, dtype, train, **null):
    from showtell_amd._lib import dtype_code, lib, ptr, stream
    a = {k: (None if k in null else ptr(v)) for k, v in t.items()}
    return lib().st_linear_bn1d_forward(a["x"], a["w"], a["bias"], a["gamma"], a["beta"], a["rm"], a["rv"], B, F, E, dtype_code(TORCH_DTYPE[dtype]),
                                        int(train), H.MOMENTUM, H.EPS, a["z"], a["mean"], a["rstd"], None, a["y"], stream())


def _backward(t, B, F, E, dtype, train, short=0, **null):
    from showtell_amd._lib import dtype_code, lib, ptr, stream
    a = {k: (None if k in null else ptr(v)) for k, v in t.items()}
    nbytes = lib().st_head_workspace_bytes(B, F, E, dtype_code(TORCH_DTYPE[dtype]))
    ws = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
    return lib().st_linear_bn1d_backward(a["dy"], a["z"], a["x"], a["gamma"], a["mean"], a["rstd"], B, F, E, dtype_code(TORCH_DTYPE[dtype]), int(train),
                                         a["dw"], a["db"], a["dg"], a["dbeta"], None if "ws" in null else ptr(ws), nbytes - short, stream())


def _untouched(t):
    torch.cuda.synchronize()
    return all((t[k] == SENTINEL).all().item() for k in ("y", "z", "dw", "db", "dg", "dbeta")) and (t["rm"] == 0).all().item() and (t["rv"] == 1).all().item()


@pytest.mark.parametrize("dtype", H.DTYPES)
def test_refusals_return_an_error_and_leave_the_outputs_untouched(dtype):
    from showtell_amd._lib import ShowTellHipError, lib
    err = lambda: lib().st_last_error().decode()
    for B, F, E, train, what in ((4, 12, 8, 1, "need F%8==0 and E%4==0 (F=12 E=8)"), (4, 16, 6, 1, "need F%8==0 and E%4==0 (F=16 E=6)"), (1, 16, 8, 1, "Expected more than 1 value per channel when training")):
        t = _raw(B, F, E, dtype)
        assert _forward(t, B, F, E, dtype, train) != 0 and what in err(), (what, err())
        assert _untouched(t), what
    B, F, E = 4, 16, 8
    t = _raw(B, F, E, dtype)
    for name in ("x", "w", "bias", "gamma", "beta", "rm", "rv", "z"):
        assert _forward(t, B, F, E, dtype, 1, **{name: True}) != 0 and "null pointer" in err(), name
    for name in ("dy", "z", "x", "gamma", "mean", "rstd", "dw", "db", "dg", "dbeta", "ws"):
        assert _backward(t, B, F, E, dtype, 1, **{name: True}) != 0 and "null pointer" in err(), name
    assert _backward(t, B, F, E, dtype, 1, short=1) != 0 and "workspace too small" in err()
    assert _untouched(t)
    # ... and the same shapes are accepted once nothing is wrong with the call (B = 1 in eval, the exact workspace size)
    assert _forward(t, B, F, E, dtype, 1) == 0 and _backward(t, B, F, E, dtype, 1) == 0
    one = _raw(1, 16, 8, dtype)
    assert _forward(one, 1, 16, 8, dtype, 0) == 0
    torch.cuda.synchronize()
    assert not (t["y"] == SENTINEL).any() and not (t["dw"] == SENTINEL).any() and not (one["y"] == SENTINEL).any()
    # through the module: torch's message for one sample in train mode, and nothing counted
    p = H.inputs("single", dtype)
    lin, bn = _modules(p, True)
    with pytest.raises(ShowTellHipError, match="Expected more than 1 value per channel when training"):
        _call(lin, bn, p["x"].cuda(), p["dy"], True, dtype)
    assert int(bn.num_batches_tracked) == 0 and torch.equal(bn.running_mean.cpu(), p["running_mean"])
