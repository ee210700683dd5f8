"""Global-norm clipping, weight decay and the non-finite guard of optim.SGD / Adam / AdamW (st_grad_sumsq + st_*_step_ex) against
the float64 torch replica of tests/_grad_clip_cases.py, whose inputs tests/test_grad_clip_inputs.py shows to have power.  The
optimizers are driven directly: the synthetic gradients are copied into opt.flat_grad through the p.grad views."""
import ctypes
import math

import pytest
import torch

from tests import _grad_clip_cases as G

pytestmark = pytest.mark.gpu

CLIP = dict(max_grad_norm=G.MAX_NORM, weight_decay=G.WEIGHT_DECAY, skip_nonfinite=True)


def _make(kind, start=None, **kw):
    from showtell_amd import optim
    ps = [torch.nn.Parameter(p.clone().cuda()) for p in (start if start is not None else G.params())]
    return getattr(optim, kind)(ps, **G.HYPER[kind], **kw)


def _set_grads(opt, step, mult=1.0):
    for p, g in zip(opt.params, step):
        assert p.grad.data_ptr() == opt.flat_grad.data_ptr() + 4 * opt.offsets[[q is p for q in opt.params].index(True)]
        p.grad.copy_(g * mult)


def _buffers(opt):
    out = {"flat": opt.flat, **opt._state()}
    if opt.shadow is not None:
        out["shadow"] = opt.shadow
    return out


def _bits(t):
    return t.detach().clone().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _assert_bit_equal(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), f"{what}: {k} differs in {(_bits(a[k]) != _bits(b[k])).sum().item()} elements"


@pytest.mark.parametrize("shadow", [None, torch.bfloat16], ids=["noshadow", "bf16shadow"])
@pytest.mark.parametrize("kind", G.KINDS)
def test_six_steps_match_the_float64_replica(kind, shadow):
    """Largest measured error / bound on an MI355X: see DESIGN.md section 7 (row 'gradient clipping')."""
    opt = _make(kind, shadow_dtype=shadow, **CLIP)
    assert opt.n == 3184
    for k, step in enumerate(G.grads()):
        _set_grads(opt, step)
        before = {n: t.clone() for n, t in _buffers(opt).items()}
        opt.step()
        if k == G.NAN_STEP:
            assert math.isinf(opt.last_grad_norm.item())
            _assert_bit_equal(before, _buffers(opt), "the skipped step")
            assert opt.skipped_steps == 1
        else:
            assert not torch.equal(before["flat"], opt.flat)
            ref = G.norms()[k]
            assert abs(opt.last_grad_norm.item() / ref - 1) <= 1e-5
            assert abs(opt.last_clip_coef.item() / min(1.0, G.MAX_NORM / (ref + 1e-6)) - 1) <= 1e-5
    err = G.rel_err(G.unpadded(opt.flat, opt.offsets), G.replica(kind))
    print(f"MEASURE {kind} shadow={shadow}: max|p - p_ref| / max|p_ref| = {err:.3e} (bound {G.BOUND:.0e})")
    assert err <= G.BOUND
    assert opt.steps == 6 and opt.skipped_steps == 1 and opt.skipped_steps.is_cuda and opt.last_grad_norm.is_cuda
    sd = opt.state_dict()
    if kind != "SGD":
        assert [ent["step"] for ent in sd["state"].values()] == [5] * len(G.SHAPES)
    if shadow is not None:
        assert torch.equal(_bits(opt.shadow), _bits(opt.flat.to(shadow)))


@pytest.mark.parametrize("kind", ["Adam", "AdamW"])
def test_three_steps_past_the_grid_cap_match_the_float64_replica(kind):
    """2048 * 1024 + 5 and 3 elements: every block of the capped grid makes a second grid-stride trip, the first tensor's
    one-element vector tail lies in it, and the step kernel's head adds up 2048 partial sums, eight per thread.
    Largest measured error / bound on an MI355X: DESIGN.md section 7 (row 'flat Adam past the grid cap')."""
    from showtell_amd._lib import lib
    opt = _make(kind, start=G.long_params(), shadow_dtype=torch.bfloat16, **CLIP)
    assert opt.n == 2097164 and opt.offsets == [0, 2097160]
    norms = [math.sqrt(sum((t.double() ** 2).sum().item() for t in step)) for step in G.long_grads()]
    for k, step in enumerate(G.long_grads()):
        _set_grads(opt, step)
        opt.step()
        assert opt._nparts.value == lib().st_grad_sumsq_max_parts() == 2048
        assert abs(opt.last_grad_norm.item() / norms[k] - 1) <= 1e-5
        assert abs(opt.last_clip_coef.item() / min(1.0, G.MAX_NORM / (norms[k] + 1e-6)) - 1) <= 1e-5
    err = G.rel_err(G.unpadded(opt.flat, opt.offsets, G.long_params()), G.replica(kind, long=True))
    print(f"MEASURE {kind} past the grid cap: max|p - p_ref| / max|p_ref| = {err:.3e} (bound {G.BOUND:.0e})")
    assert err <= G.BOUND
    assert opt.steps == 3 and opt.skipped_steps == 0
    assert torch.equal(_bits(opt.shadow), _bits(opt.flat.to(torch.bfloat16)))
    pad = torch.ones(opt.n, dtype=torch.bool)
    for p, o in zip(opt.params, opt.offsets):
        pad[o:o + p.numel()] = False
    assert pad.sum() == 4 and (opt.flat.cpu()[pad] == 0).all()                     # the padding elements stay what they were


@pytest.mark.parametrize("kind", ["SGD", "Adam"])
def test_the_clip_coefficient_is_all_that_differs_from_the_plain_step(kind):
    """Without weight decay the new path must be the old kernel with grad_scale = the coefficient it reports: bit for bit, on
    a first and on a later step, clipped 74 -> 5 and 2236 -> 5."""
    from showtell_amd._lib import check, lib, ptr, stream
    opt = _make(kind, shadow_dtype=torch.bfloat16, max_grad_norm=G.MAX_NORM)
    old = {n: t.clone() for n, t in _buffers(opt).items()}
    old_grad = torch.empty_like(opt.flat_grad)
    for k, step in enumerate((G.grads()[0], G.grads()[2])):
        _set_grads(opt, step)
        opt.step()
        coef = opt.last_clip_coef.item()
        assert 0 < coef < 1
        old_grad.copy_(opt.flat_grad)
        if kind == "SGD":
            check(lib().st_sgd_step(ptr(old["flat"]), ptr(old_grad), ptr(old["momentum_buffer"]), ptr(old["shadow"]), opt.n, 0.05, 0.9,
                                    int(k == 0), coef, stream()), "st_sgd_step")
        else:
            check(lib().st_adam_step(ptr(old["flat"]), ptr(old_grad), ptr(old["exp_avg"]), ptr(old["exp_avg_sq"]), ptr(old["shadow"]), opt.n,
                                     1e-3, 0.9, 0.999, 1e-8, k + 1, coef, stream()), "st_adam_step")
        _assert_bit_equal(old, _buffers(opt), f"{kind} step {k + 1}")


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("kind", G.KINDS)
def test_a_max_norm_far_above_the_norm_changes_no_bit(kind, grad_scale):
    wd = {"weight_decay": 0.0} if kind == "AdamW" else {}        # the decay itself is not what is compared here
    plain, huge = _make(kind, **wd), _make(kind, max_grad_norm=1e30, **wd)
    for step in (G.grads()[0], G.grads()[2], G.grads()[3]):
        for opt in (plain, huge):
            opt.grad_scale = grad_scale
            _set_grads(opt, step)
            opt.step()
        assert huge.last_clip_coef.item() == grad_scale
    _assert_bit_equal(_buffers(plain), _buffers(huge), kind)
    assert plain.last_grad_norm.item() == 0.0                      # the default optimizer never launched the norm


def _norm_via_c_abi(x, max_norm=5.0, lr=0.5):
    """st_grad_sumsq + st_sgd_step_ex on a raw n (no padding to 4): returns (norm bits, norm, coef, nparts, updated param)."""
    from showtell_amd._lib import check, lib, ptr, stream
    L = lib()
    n = x.numel()
    partials = torch.full((L.st_grad_sumsq_max_parts(),), float("nan"), device="cuda")
    status = torch.zeros(8, device="cuda", dtype=torch.int32)
    param = torch.zeros(n + 4, device="cuda")                      # four guard elements behind the last one
    nparts = ctypes.c_int(-1)
    check(L.st_grad_sumsq(ptr(x), n, ptr(partials), ctypes.byref(nparts), stream()), "st_grad_sumsq")
    check(L.st_sgd_step_ex(ptr(param), ptr(x), None, None, n, lr, 0.0, 1, 1.0, ptr(partials), nparts.value, max_norm, 0.0, 0, 0,
                           ptr(status), stream()), "st_sgd_step_ex")
    st = status.cpu()
    assert st[2:].tolist() == [1, 0, 0, 1, 0, 0]                   # applied 1, skipped 0; slot 0 read, slot 1 written
    assert torch.isnan(partials[nparts.value:]).all() and (param[n:] == 0).all()
    f = st.view(torch.float32)
    return st[0].item(), f[0].item(), f[1].item(), nparts.value, param[:n]


def _norm_cases():
    from showtell_amd._lib import lib
    return [1, 3, 4, 5, 1023, 1024, 1025, lib().st_grad_sumsq_max_parts() * 256 * 4 + 5]


@pytest.mark.parametrize("big", [False, True], ids=["normal", "one_1e18"])
def test_norm_accuracy_and_shapes(big):
    """Relative error of the norm <= 1e-5: the longest chain is a few tens of fp32 roundings of 6e-8, halved by the square root.
    Measured on an MI355X: DESIGN.md section 7."""
    from showtell_amd._lib import lib
    max_parts = lib().st_grad_sumsq_max_parts()
    worst = 0.0
    for n in _norm_cases():
        x = torch.randn(n, generator=torch.Generator().manual_seed(n))
        if big:
            x[n // 2] = 1e18
        ref = x.double().norm().item()
        xg = x.cuda()
        bits, norm, coef, nparts, param = _norm_via_c_abi(xg)
        assert nparts == min(max((n // 4 + 255) // 256, 1), max_parts)      # the step kernels' grid: a function of n alone
        err = abs(norm / ref - 1)
        worst = max(worst, err)
        print(f"MEASURE n={n} big={big}: norm {norm:.8g} ref {ref:.8g} rel err {err:.2e}, nparts {nparts}")
        assert err <= 1e-5
        want = min(1.0, 5.0 / (ref + 1e-6))
        assert abs(coef / want - 1) <= 1e-6
        assert _norm_via_c_abi(xg)[0] == bits                      # the same input, the same bits
        # the update itself on a length that is no multiple of the vector: p = 0 - lr * coef * g
        assert torch.allclose(param.cpu().double(), -0.5 * want * x.double(), rtol=1e-5, atol=0)
    print(f"MEASURE worst relative norm error, big={big}: {worst:.2e}")


@pytest.mark.parametrize("kind", G.KINDS)
def test_data_parallel_scale_clips_the_norm_of_the_average(kind):
    """flat_grad holds the sum over two ranks, grad_scale = 1/2: the same norms and parameters as the world-1 run."""
    one, two = _make(kind, shadow_dtype=None, **CLIP), _make(kind, shadow_dtype=None, **CLIP)
    two.grad_scale = 0.5
    for k, step in enumerate(G.grads()):
        _set_grads(one, step)
        _set_grads(two, step, 2.0)
        one.step(); two.step()
        n1, n2 = one.last_grad_norm.item(), two.last_grad_norm.item()
        if k == G.NAN_STEP:
            assert math.isinf(n1) and math.isinf(n2)
            continue
        assert abs(n2 / n1 - 1) <= G.BOUND and abs(n2 / G.norms()[k] - 1) <= 1e-5
        assert abs(two.last_clip_coef.item() / (0.5 * one.last_clip_coef.item()) - 1) <= G.BOUND
    ref = G.replica(kind)
    e1, e2 = G.rel_err(G.unpadded(one.flat, one.offsets), ref), G.rel_err(G.unpadded(two.flat, two.offsets), ref)
    e12 = G.rel_err(G.unpadded(two.flat, two.offsets), G.unpadded(one.flat, one.offsets))
    print(f"MEASURE {kind}: world 1 {e1:.3e}, world 2 {e2:.3e}, between them {e12:.3e}")
    assert e2 <= G.BOUND and e12 <= G.BOUND


@pytest.mark.parametrize("kind", G.KINDS)
def test_without_the_guard_a_non_finite_norm_propagates(kind):
    """torch's behaviour with error_if_nonfinite=False: the coefficient is max / inf = 0 and 0 * inf is NaN."""
    opt = _make(kind, shadow_dtype=None, max_grad_norm=G.MAX_NORM, weight_decay=G.WEIGHT_DECAY)
    for step in G.grads()[:G.NAN_STEP + 1]:
        _set_grads(opt, step)
        opt.step()
    assert math.isinf(opt.last_grad_norm.item()) and opt.last_grad_norm.item() > 0
    assert opt.skipped_steps == 0
    assert not torch.isfinite(opt.flat).all()
    o = opt.offsets[G.INF_AT[0]] + G.INF_AT[1]
    assert not math.isfinite(opt.flat[o].item())
    torch.cuda.synchronize()                                       # a NaN in a buffer is a value, not a device fault


def test_checkpoint_round_trip_through_torch_adamw_and_resume():
    from showtell_amd import optim
    full = _make("AdamW", **CLIP)
    for step in G.grads():
        _set_grads(full, step)
        full.step()
    first = _make("AdamW", **CLIP)
    for step in G.grads()[:3]:
        _set_grads(first, step)
        first.step()
    sd = first.state_dict()
    g0 = sd["param_groups"][0]
    assert g0["weight_decay"] == G.WEIGHT_DECAY and g0["decoupled_weight_decay"] is True and g0["max_grad_norm"] == G.MAX_NORM and g0["skip_nonfinite"] is True
    assert [ent["step"] for ent in sd["state"].values()] == [2] * len(G.SHAPES)          # three calls, one skipped
    ref_opt = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(s)) for s in G.SHAPES], lr=1.0, weight_decay=0.5)
    ref_opt.load_state_dict(sd)
    rg = ref_opt.param_groups[0]
    assert rg["weight_decay"] == G.WEIGHT_DECAY and rg["decoupled_weight_decay"] is True and rg["lr"] == 1e-3
    # ... and back, into an optimizer built with other settings
    second = optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in first.params], lr=1.0)
    assert second.param_groups[0]["decoupled_weight_decay"] is False and second.max_grad_norm is None
    second.load_state_dict(ref_opt.state_dict())
    sg = second.param_groups[0]
    assert (sg["lr"], sg["weight_decay"], sg["decoupled_weight_decay"], sg["max_grad_norm"], second.skip_nonfinite) == (1e-3, G.WEIGHT_DECAY, True, G.MAX_NORM, True)
    assert second.steps == 2
    _assert_bit_equal(_buffers(first), _buffers(second), "the restore")
    for step in G.grads()[3:]:
        _set_grads(second, step)
        second.step()
    _assert_bit_equal(_buffers(full), _buffers(second), "3 + save + load + 3 against 6 uninterrupted")
    assert second.state_dict()["state"][0]["step"] == 5
    # a default optimizer's checkpoint keeps the key set it had before these keywords existed
    assert set(_make("SGD").state_dict()["param_groups"][0]) == {"lr", "momentum", "dampening", "weight_decay", "nesterov", "params"}
    assert set(_make("Adam").state_dict()["param_groups"][0]) == {"lr", "betas", "eps", "weight_decay", "amsgrad", "params"}


def test_param_group_changes_are_honoured_like_lr():
    opt = _make("SGD", shadow_dtype=None)
    ref = _make("SGD", shadow_dtype=None, max_grad_norm=G.MAX_NORM, weight_decay=G.WEIGHT_DECAY)
    opt.param_groups[0]["max_grad_norm"] = G.MAX_NORM
    opt.param_groups[0]["weight_decay"] = G.WEIGHT_DECAY
    for o in (opt, ref):
        _set_grads(o, G.grads()[0])
        o.step()
    _assert_bit_equal(_buffers(ref), _buffers(opt), "hyper-parameters set through param_groups")
    assert opt.last_clip_coef.item() < 0.1


# ---- through the Trainer ------------------------------------------------------------------------------------------------

E = H = 64
L, V, B = 2, 120, 4


def _trainer(**kw):
    from showtell_amd import optim
    from showtell_amd.cnn import ResNet
    from showtell_amd.rnn import RNN
    from showtell_amd.train import Trainer
    torch.manual_seed(21)
    cnn, rnn = ResNet(18, E).cuda().train(), RNN(E, H, V, L).cuda().train()
    opt = optim.Adam(Trainer.trainable_params(cnn, rnn), lr=1e-3, shadow_dtype=None, **kw)
    return Trainer(cnn, rnn, opt), opt


def test_trainer_reports_the_norm_and_a_huge_max_norm_equals_the_default_run():
    """The gradient kernels sum with fp32 atomics, so two runs on the same data differ in the last bits of the GRADIENT
    (tests/test_gpu_optim_state.py).  The comparison is between optimizers, so the default run is handed the gradients the
    max_grad_norm = 1e30 run computed (flat_grad overwritten just before each of its optimizer steps): then every bit must agree."""
    from showtell_amd.train import synthetic_batch
    data = [synthetic_batch(B, V, seed=60 + i, image_size=96, mean=6, std=1.5, lo=4, hi=9) for i in range(3)]
    tr, opt = _trainer(max_grad_norm=1.0)
    assert tr.grad_norm.data_ptr() == opt.last_grad_norm.data_ptr() and tr.grad_norm.is_cuda
    for d in data:
        tr.step(*d)
    tr.flush()
    got, ref = tr.grad_norm.item(), opt.flat_grad.double().norm().item()
    print(f"MEASURE trainer grad norm {got:.8g}, float64 norm of flat_grad {ref:.8g}, coef {opt.last_clip_coef.item():.6g}")
    assert math.isfinite(got) and got > 0 and abs(got / ref - 1) <= 1e-5
    assert opt.skipped_steps == 0

    recorded = []
    tr_h, opt_h = _trainer(max_grad_norm=1e30)
    step_h = opt_h.step
    opt_h.step = lambda: (recorded.append(opt_h.flat_grad.clone()), step_h())[1]
    tr_d, opt_d = _trainer()
    assert tr_d.grad_norm is not None and torch.equal(_bits(opt_d.flat), _bits(opt_h.flat))
    step_d = opt_d.step
    opt_d.step = lambda: (opt_d.flat_grad.copy_(recorded[opt_d.steps]), step_d())[1]
    for t in (tr_h, tr_d):
        for d in data:
            t.step(*d)
        t.flush()
    assert len(recorded) == 3 and opt_h.steps == opt_d.steps == 3
    assert opt_h.last_clip_coef.item() == 1.0
    _assert_bit_equal(_buffers(opt_d), _buffers(opt_h), "default run against max_grad_norm = 1e30")
