"""The bf16 soft-attention training step bench.py times (BASELINE configs[2], `attention_gru_bs64_*`), against a float64
oracle (R.attn_train_loss on bf16-representable weights and features).

A  one configs[2] step on the fused route: RNN_Attn.loss -> backward -> optim.SGD(momentum) with its bf16 shadow, GRU and
   LSTM, B = 64 and a ragged B = 37: loss, alphas, every gradient, every update, every bf16 working copy after the step.
B  the same step written as Attention/main_attn.py:126-133 writes it (forward() -> nn.CrossEntropyLoss + alpha term).
C  B = 520: the early steps have >= 512 rows (256-thread workgroups, the G == 1 paths of attn_fwd_kernel / attn_bwd_kernel),
   the later ones fewer (1024 threads), in one backward; bf16 and fp32.
D  a second step from the GPU's own state after A (fp32 parameters, bf16 working copies, momentum buffer).
E  gradient semantics: an upstream gradient of 0.25, and two backward() calls accumulating into .grad.

Inputs: post-ReLU features |randn| with a random per-pixel gain (so z depends on which pixel wins) and attn.full_att.weight
scaled by FULL_ATT_SCALE, so that attention is clearly peaked but not saturated.

Each bound has the worst value measured on the MI355X over every case next to it (margin about 2x).
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import restatement as R
from tests.test_gpu_attention import _make
from tests.test_gpu_decoder_bench_shape import (_bf16, _bf16_params, _captions, _check_grads, _check_update, _rel_l2,
                                                _rel_max)

pytestmark = pytest.mark.gpu

E = H = A = 512
FD, P = 2048, 49
LR, MOM = 0.5, 0.9
FULL_ATT_SCALE = 8.0    # float64 oracle, B = 64 GRU: median per-row max alpha 0.17, largest 0.64 (uniform: 0.020)
# rows per attention step at which attn_fwd_launch / attn_bwd_launch (csrc/attn_kernels.hip) switch from 1024-thread to
# 256-thread workgroups; at F = 2048, A = 512 the 256-thread kernels take their G == 1 code paths
WIDE_ROWS = 512

# bounds; measured worst on the MI355X after the "#"
LOSS_REL = 5e-3         # bf16 loss: 4.2e-5
GRAD_L2 = 3e-2          # bf16 gradients and SGD updates beyond one fp32 ulp: 1.5e-2 (init_h.weight, LSTM)
GRAD_MAX = 6e-2         # 2.4e-2 (encoder_att.weight)
# attn.decoder_att.weight in bf16: d att2 is summed over 49 pixels of d u = d e_p w_f lrelu'(att1_p + att2), and with peaked
# attention each d e_p carries the bf16 storage rounding of att1 and h; the same restatement in fp32 (case C fp32, E fp32)
# measures <= 4.7e-5, so the kernels' arithmetic is not the source.  Measured 5.3e-2 (rel L2), 2.1e-1 (rel max, A gru B=64)
DEC_ATT_L2 = 1e-1
DEC_ATT_MAX = 4e-1
ALPHA_L2 = 1e-2         # bf16 alphas of the live steps: 4.8e-3
ALPHA_MAX = 4e-2        # 6.9e-3
ROW_SUM = 2e-3          # |sum_p alpha - 1| of a live step, any dtype: 2.0e-7
BIAS_CANCEL = 1e-2      # |d full_att.bias| (and its update) over the sum sum_p |d e_p| it cancels: 2.2e-8
F32_L2 = 1e-4           # fp32: loss, alphas, gradients: 4.7e-5
F32_MAX = 4e-4          # 1.9e-4 (encoder_att.weight, C lstm)
ROUTE_L2 = 1e-2         # B: drop-in route against the fused route, same inputs, bf16: 2.3e-3
ROUTE_MAX = 4e-2        # 2.0e-3
ACCUM_L2 = 1e-5         # E: accumulated .grad against the sum of the two separately computed gradients: 1.9e-7
ACCUM_MAX = 1e-5        # 3.4e-7


def _features(B, seed, dtype, Fd=FD):
    """(B, F, P) post-ReLU features with a per-(sample, pixel) gain"""
    g = torch.Generator().manual_seed(seed)
    gain = 0.75 + 0.5 * torch.rand(B, 1, P, generator=g)
    x = torch.randn(B, Fd, P, generator=g).abs() * gain
    return _bf16(x) if dtype == torch.bfloat16 else x


def _params(cell, V, L, seed, dtype, Ed=E, Fd=FD, Ad=A):
    sd = R.init_decoder_params(Ed, Ed, V, L, cell, seed=seed, attn=dict(F=Fd, A=Ad))
    sd["attn.full_att.weight"] *= FULL_ATT_SCALE
    return _bf16_params(sd) if dtype == torch.bfloat16 else sd


def _ragged_lens_37():
    """B = 37: every length 6..25 once, a run of six 12s, sorted descending"""
    rng = np.random.RandomState(37)
    lens = list(range(6, 26)) + [12] * 6 + [int(v) for v in rng.randint(6, 26, size=11)]
    lens = sorted(lens, reverse=True)
    assert len(lens) == 37 and min(lens) == 6 and max(lens) == 25 and lens.count(12) >= 6
    return lens


def _lens_520():
    """B = 520, lengths 4..9: steps 0..3 have 520 rows, the later ones fewer than 512"""
    rng = np.random.RandomState(520)
    lens = sorted([int(v) for v in rng.randint(4, 10, size=520)], reverse=True)
    assert set(lens) == set(range(4, 10))
    return lens


def _oracle(params, feat, cap, lens, cell, monkeypatch, scale=1.0):
    """float64 R.attn_train_loss -> backward.  Returns (loss, alphas, grads, cancelled): `cancelled` is sum |d e_p| over every
    (row, step, pixel), the sum that d full_att.bias = sum d e_p cancels (softmax is shift invariant), read from a hook on
    the scores that torch.softmax receives."""
    po = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    parts = []
    softmax = torch.softmax

    def hooked(x, dim):
        if x.requires_grad:
            x.register_hook(lambda g: parts.append(g.abs().sum().item()))
        return softmax(x, dim)
    with monkeypatch.context() as mp:
        mp.setattr(torch, "softmax", hooked)
        lo, _, al = R.attn_train_loss(po, feat.double(), cap, lens, 1.0, cell)
        (scale * lo).backward()
    return lo.item(), al.detach(), {k: p.grad for k, p in po.items()}, sum(parts)


def _live(al, lens):
    return torch.cat([al[b, :l] for b, l in enumerate(lens)], 0)


def _check_loss(got, ref, tag, bound):
    err = abs(got - ref) / abs(ref)
    print(f"MEASURE {tag} loss: rel {err:.2e} (bound {bound:.0e})")
    assert err < bound, (tag, got, ref)


def _check_alphas(alphas, ref, lens, tag, l2_bound, max_bound):
    """live steps against the oracle; rows of a live step sum to one; padded steps are exactly zero (rnn_attn.py:65)"""
    al = alphas.detach().double().cpu()
    live, live_ref = _live(al, lens), _live(ref, lens)
    l2, mx = _rel_l2(live, live_ref), _rel_max(live, live_ref)
    rs = (live.sum(1) - 1).abs().max().item()
    peak = live_ref.max(1)[0]
    print(f"MEASURE {tag} alphas: rel_l2 {l2:.2e} rel_max {mx:.2e} |row sum - 1| {rs:.2e}; "
          f"oracle max alpha per row: median {peak.median():.3f} largest {peak.max():.3f} (uniform {1 / P:.3f})")
    assert l2 < l2_bound and mx < max_bound and rs < ROW_SUM, (tag, l2, mx, rs)
    for b, l in enumerate(lens):
        assert (al[b, l:] == 0).all(), (tag, b, l)


def _check_bias(grad, cancelled, tag, update_err=None):
    """d full_att.bias is analytically zero: bound it, or the error of its SGD update over LR, by the sum it cancels"""
    if update_err is None:
        r, what = grad.abs().max().item() / cancelled, "|grad|"
    else:
        r, what = update_err.abs().max().item() / (LR * cancelled), "|update - oracle update|"
    print(f"MEASURE {tag} attn.full_att.bias: {what} {r:.2e} of the cancelled sum {cancelled:.3e}")
    assert r < BIAS_CANCEL, (tag, r)


def _check_all_grads(grads, ref, cancelled, tag, l2_bound, max_bound):
    for k, g in grads.items():
        if k == "attn.full_att.bias":
            _check_bias(g, cancelled, f"{tag} grad")
        elif k == "attn.decoder_att.weight" and l2_bound == GRAD_L2:
            _check_grads(g, ref[k], f"{tag} grad {k}", DEC_ATT_L2, DEC_ATT_MAX)
        else:
            _check_grads(g, ref[k], f"{tag} grad {k}", l2_bound, max_bound)


def _shadowed(m):
    """{name: shadow} for every parameter the kernels read as a bf16 working copy (RNN_Attn._c_params, wc())"""
    shadows = {k: p._st_shadow for k, p in m.named_parameters() if getattr(p, "_st_shadow", None) is not None}
    bits = {k: s.view(torch.int16).clone() for k, s in shadows.items()}     # before _c_params could refresh anything
    _, keep = m._c_params()
    read = {t.data_ptr() for t in keep}
    out = {k: bits[k] for k, s in shadows.items() if s.data_ptr() in read}
    assert len(out) == len(read), "a working copy the kernels read is not the optimizer's bf16 shadow"
    return out


def _check_shadows(m, tag):
    """after optim.SGD.step: each working copy is the round-to-nearest-even bf16 of the new fp32 value, bit for bit"""
    sh = _shadowed(m)
    named = dict(m.named_parameters())
    bad = {k: int((b != named[k].detach().bfloat16().view(torch.int16)).sum()) for k, b in sh.items()}
    print(f"MEASURE {tag} bf16 shadows: {len(sh)} working copies, elements differing from RNE(bf16(fp32)): {sum(bad.values())}")
    assert not any(bad.values()), (tag, {k: v for k, v in bad.items() if v})
    return set(sh)


def _gpu_step(m, opt, feat, cap, lens):
    """zero_grad -> loss -> backward -> step.  Returns (loss, alphas, before, grads, after) on the host, float64."""
    named = list(m.named_parameters())
    before = {k: p.detach().double().cpu().clone() for k, p in named}
    with torch.no_grad():
        _, alphas = m(feat.cuda(), cap.cuda(), lens)
    opt.zero_grad()
    loss = m.loss(feat.cuda(), cap.cuda(), lens, 1.0)
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().double().cpu().clone() for k, p in named}
    opt.step()
    torch.cuda.synchronize()
    after = {k: p.detach().double().cpu().clone() for k, p in named}
    return loss.item(), alphas.cpu(), before, grads, after


def _check_updates(before, after, grads_ref, bufs, cancelled, tag):
    """torch.optim.SGD(lr, momentum) from `before` with the oracle's gradient and the GPU's momentum buffer (None: first step)"""
    for k, g in grads_ref.items():
        ref = before[k].clone()
        R.sgd_momentum_step(ref, g, None if bufs is None else bufs[k].clone(), LR, MOM)
        if k == "attn.full_att.bias":
            _check_bias(None, cancelled, f"{tag} update", after[k] - ref)
        else:
            bounds = (DEC_ATT_L2, DEC_ATT_MAX) if k == "attn.decoder_att.weight" else (GRAD_L2, GRAD_MAX)
            _check_update(after[k], before[k], ref, f"{tag} update {k}", *bounds)


def _batch(B, V, seed):
    if B == 37:
        return _captions(_ragged_lens_37(), V, seed)
    return R.synthetic_captions(B, V, seed=seed)


# ====================================================================================================================
# A. one configs[2] training step, fused route
# ====================================================================================================================

@pytest.mark.parametrize("B", [64, 37])
@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_configs2_bf16_training_step_matches_fp64_oracle(cell, B, monkeypatch):
    from showtell_amd import optim
    V, L, seed = 10000, 5, 200 + B
    params = _params(cell, V, L, seed, torch.bfloat16)
    feat = _features(B, seed, torch.bfloat16)
    cap, lens = _batch(B, V, seed)
    m = _make(cell, params, torch.bfloat16).train()
    opt = optim.SGD(list(m.parameters()), lr=LR, momentum=MOM)
    loss, alphas, before, grads, after = _gpu_step(m, opt, feat, cap, lens)
    lo, al_o, g_o, cancelled = _oracle(params, feat, cap, lens, cell, monkeypatch)
    tag = f"A {cell} B={B}"
    _check_loss(loss, lo, tag, LOSS_REL)
    _check_alphas(alphas, al_o, lens, tag, ALPHA_L2, ALPHA_MAX)
    _check_all_grads(grads, g_o, cancelled, tag, GRAD_L2, GRAD_MAX)
    _check_updates(before, after, g_o, None, cancelled, tag)
    _check_shadows(m, tag)


# ====================================================================================================================
# B. the same step, written as Attention/main_attn.py:126-133 writes it
# ====================================================================================================================

def test_configs2_dropin_route_matches_oracle_and_fused_route(monkeypatch):
    cell, B, V, L, seed = "gru", 64, 10000, 5, 264
    params = _params(cell, V, L, seed, torch.bfloat16)
    feat = _features(B, seed, torch.bfloat16).cuda()
    cap, lens = _batch(B, V, seed)
    cap = cap.cuda()
    m = _make(cell, params, torch.bfloat16).train()
    target = nn.utils.rnn.pack_padded_sequence(cap, lens, batch_first=True)[0]
    logits, alphas = m(feat, cap, lens)
    loss = nn.CrossEntropyLoss()(logits, target)
    loss = loss + 1.0 * ((1. - alphas.sum(dim=1)) ** 2).mean()
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().double().cpu().clone() for k, p in m.named_parameters()}
    mf = _make(cell, params, torch.bfloat16).train()
    mf.loss(feat, cap, lens, 1.0).backward()
    torch.cuda.synchronize()
    fused = {k: p.grad.detach().double().cpu() for k, p in mf.named_parameters()}
    lo, al_o, g_o, cancelled = _oracle(params, feat.cpu(), cap.cpu(), lens, cell, monkeypatch)
    tag = f"B {cell} B={B} drop-in"
    _check_loss(loss.item(), lo, tag, LOSS_REL)
    _check_alphas(alphas, al_o, lens, tag, ALPHA_L2, ALPHA_MAX)
    _check_all_grads(grads, g_o, cancelled, tag, GRAD_L2, GRAD_MAX)
    for k, g in grads.items():
        if k == "attn.full_att.bias":
            continue
        l2, mx = _rel_l2(g, fused[k]), _rel_max(g, fused[k])
        print(f"MEASURE {tag} vs fused route {k}: rel_l2 {l2:.2e} rel_max {mx:.2e}")
        assert l2 < ROUTE_L2 and mx < ROUTE_MAX, (k, l2, mx)


# ====================================================================================================================
# C. both workgroup shapes of the attention kernels in one backward
# ====================================================================================================================

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_wide_and_narrow_attention_steps_match_fp64_oracle(cell, dtype, monkeypatch):
    B, V, L, seed = 520, 1000, 2, 520
    lens = _lens_520()
    rows = R.batch_sizes(lens)
    print(f"MEASURE C rows per step: {rows}")
    assert any(r >= WIDE_ROWS for r in rows) and any(r < WIDE_ROWS for r in rows), rows
    cap, lens = _captions(lens, V, seed)
    params = _params(cell, V, L, seed, dtype)
    feat = _features(B, seed, dtype)
    m = _make(cell, params, dtype).train()
    with torch.no_grad():
        _, alphas = m(feat.cuda(), cap.cuda(), lens)
    loss = m.loss(feat.cuda(), cap.cuda(), lens, 1.0)
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().double().cpu() for k, p in m.named_parameters()}
    lo, al_o, g_o, cancelled = _oracle(params, feat, cap, lens, cell, monkeypatch)
    tag = f"C {cell} {'fp32' if dtype == torch.float32 else 'bf16'} B={B}"
    f32 = dtype == torch.float32
    _check_loss(loss.item(), lo, tag, F32_L2 if f32 else LOSS_REL)
    _check_alphas(alphas, al_o, lens, tag, *((F32_L2, F32_MAX) if f32 else (ALPHA_L2, ALPHA_MAX)))
    _check_all_grads(grads, g_o, cancelled, tag, *((F32_L2, F32_MAX) if f32 else (GRAD_L2, GRAD_MAX)))


# ====================================================================================================================
# D. a second step from the GPU's own state
# ====================================================================================================================

@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_configs2_second_step_from_gpu_state_matches_fp64_oracle(cell, monkeypatch):
    """Step 2's oracle starts from what the GPU holds after step 1: its fp32 parameters, rounded to bf16 where the kernels
    read a bf16 working copy, and its momentum buffer.  So step 2 is checked on its own, and a working copy or momentum
    buffer that step 1 left stale shows as a step-2 error."""
    from showtell_amd import optim
    B, V, L, seed = 64, 10000, 5, 264
    params = _params(cell, V, L, seed, torch.bfloat16)
    m = _make(cell, params, torch.bfloat16).train()
    opt = optim.SGD(list(m.parameters()), lr=LR, momentum=MOM)
    cap1, lens1 = _batch(B, V, seed)
    _gpu_step(m, opt, _features(B, seed, torch.bfloat16), cap1, lens1)
    shadowed = _check_shadows(m, f"D {cell} step 1")
    names = [k for k, _ in m.named_parameters()]
    state = opt.state_dict()["state"]
    bufs = {k: state[i]["momentum_buffer"].double().cpu() for i, k in enumerate(names)}
    cap2, lens2 = _batch(B, V, seed + 1)
    feat2 = _features(B, seed + 1, torch.bfloat16)
    loss, alphas, before, grads, after = _gpu_step(m, opt, feat2, cap2, lens2)
    start = {k: (_bf16(v) if k in shadowed else v) for k, v in before.items()}
    lo, al_o, g_o, cancelled = _oracle(start, feat2, cap2, lens2, cell, monkeypatch)
    tag = f"D {cell} B={B} step 2"
    _check_loss(loss, lo, tag, LOSS_REL)
    _check_alphas(alphas, al_o, lens2, tag, ALPHA_L2, ALPHA_MAX)
    _check_all_grads(grads, g_o, cancelled, tag, GRAD_L2, GRAD_MAX)
    _check_updates(before, after, g_o, bufs, cancelled, tag)
    _check_shadows(m, tag)


# ====================================================================================================================
# E. gradient semantics: upstream gradient != 1, accumulation over backward() calls
# ====================================================================================================================

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_scaled_and_accumulated_gradients(cell, dtype, monkeypatch):
    Ed, Fd, V, L, seed = 128, 256, 500, 2, 300
    params = _params(cell, V, L, seed, dtype, Ed=Ed, Fd=Fd, Ad=Ed)
    feat1, feat2 = _features(12, seed, dtype, Fd), _features(9, seed + 1, dtype, Fd)
    cap1, lens1 = _captions([14, 12, 12, 12, 11, 9, 9, 8, 7, 6, 5, 4], V, seed)
    cap2, lens2 = _captions([10, 10, 9, 8, 8, 6, 5, 5, 3], V, seed + 1)
    m = _make(cell, params, dtype).train()

    def run(feat, cap, lens, scale, zero):
        if zero:
            for p in m.parameters():
                p.grad = None
        loss = m.loss(feat.cuda(), cap.cuda(), lens, 1.0)
        (loss if scale == 1.0 else scale * loss).backward()
        torch.cuda.synchronize()
        return {k: p.grad.detach().double().cpu().clone() for k, p in m.named_parameters()}
    ga = run(feat1, cap1, lens1, 0.25, True)
    gacc = run(feat2, cap2, lens2, 1.0, False)          # no zero_grad: accumulates into .grad
    gb = run(feat2, cap2, lens2, 1.0, True)
    _, _, g1, c1 = _oracle(params, feat1, cap1, lens1, cell, monkeypatch, scale=0.25)
    _, _, g2, c2 = _oracle(params, feat2, cap2, lens2, cell, monkeypatch)
    f32 = dtype == torch.float32
    bounds = (F32_L2, F32_MAX) if f32 else (GRAD_L2, GRAD_MAX)
    tag = f"E {cell} {'fp32' if f32 else 'bf16'}"
    _check_all_grads(ga, g1, c1, f"{tag} 0.25 * loss", *bounds)
    _check_all_grads(gacc, {k: g1[k] + g2[k] for k in g1}, c1 + c2, f"{tag} accumulated", *bounds)
    for k in gacc:
        if k == "attn.full_att.bias":
            continue
        l2, mx = _rel_l2(gacc[k], ga[k] + gb[k]), _rel_max(gacc[k], ga[k] + gb[k])
        print(f"MEASURE {tag} accumulated vs sum of the two {k}: rel_l2 {l2:.2e} rel_max {mx:.2e}")
        assert l2 < ACCUM_L2 and mx < ACCUM_MAX, (k, l2, mx)
