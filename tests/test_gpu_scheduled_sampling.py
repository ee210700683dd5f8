"""Scheduled sampling on the GPU (st_sample_mix_rows, st_rnn_sched_inputs, st_attn_sched_inputs, input_ids of st_rnn_forward /
st_rnn_backward; scheduled_inputs, loss(input_ids=), loss(scheduled_sampling=), Trainer(scheduled_sampling=)).  The kernels hold
no generator: the caller's uniforms decide every coin and every draw, so every check is deterministic.

1  st_sample_mix_rows against st_sample_rows on the same logits and draw_u: replaced rows bit for bit, the others the teacher's
   token; coin == p, p = 0, p = 1; the three routes (register rows, 16-byte loads over memory, scalar loads)
2  p = 1 against ``sample`` with the same draws: the same ids bit for bit, both plain and both attention cells
3  the float64 oracle walks the GPU's own mixed tokens: the interval rule of tests/test_gpu_sample.py on every replaced slot,
   `replaced` the rule exactly, the caption everywhere else
4  loss(input_ids = X), X random: loss and every gradient against the float64 torch replica, also with dropout and with weights
   plus label smoothing; the embedding rows of tokens only the targets hold get exactly zero
5  input_ids = None never reaches the roll-in entry points and hands the C calls a NULL input_ids; input_ids = caption is the plain call
6  same seed or same uniforms, same tensors; the roll-in allocates and synchronises nothing
7  the Trainer's step is scheduled_inputs + loss(input_ids=) + backward + step; a callable schedule is asked with 0, 1, ..

Cases, oracles and bounds: tests/_scheduled_sampling_cases.py; tests/test_scheduled_sampling_inputs.py shows on the CPU that
they catch the seeded faults.  Each figure is printed (MEASURE ...) before it is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _scheduled_sampling_cases as K
from tests.test_gpu_sample import ROWS_LD, ROWS_V, _ptr, _sample_rows, route_inputs, rows_inputs

pytestmark = pytest.mark.gpu
END, START = 2, 1
_MODELS = {}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _model(case, which):
    """which: 'rollin' (sharpened projection) or 'loss' (the parameters of tests/_label_smoothing_cases.py)"""
    if (case, which) not in _MODELS:
        from tests.test_gpu_attention import _make as make_attn
        from tests.test_gpu_decoder import _make_sized
        family, cell, _, E, H, V, L, _ = K.CASES[case]
        params = K.rollin_params(case) if which == "rollin" else K.inputs(case)[0]
        if family == "attn":
            m = make_attn(cell, {k: v.clone() for k, v in params.items()}, torch.float32).train()
        else:
            m = _make_sized(cell, params, K.torch_dtype(case), E, H, V, L)
        _MODELS[(case, which)] = m
    return _MODELS[(case, which)]


# ====================================================================================================================
# 1: st_sample_mix_rows
# ====================================================================================================================

def _mix_rows(logits, u, coin, p, teacher, lens, step, inv_t, k, V, stride=3, t=1):
    from showtell_amd._lib import check, lib
    n, dev = logits.shape[0], logits.device
    ids = torch.full((n, stride), -7, device=dev, dtype=torch.long)
    mixed = torch.full((n, stride), -7, device=dev, dtype=torch.long)
    rep = torch.full((n, stride), 9, device=dev, dtype=torch.uint8)
    logp = torch.full((n, stride), 7.0, device=dev)
    cur = torch.full((n,), -7, device=dev, dtype=torch.long)
    # teacher (n, 4): column 2 is read; coin (n, 2): column 1
    check(lib().st_sample_mix_rows(_ptr(logits), logits.stride(0), n, V, _ptr(u), 1, float(inv_t), int(k), _ptr(coin[:, 1:]), 2, float(p),
                                   _ptr(teacher), 4, 2, _ptr(lens), int(step), _ptr(ids), _ptr(logp), _ptr(mixed), _ptr(rep), stride, t,
                                   _ptr(cur), _stream()), "st_sample_mix_rows")
    torch.cuda.synchronize()
    return ids.cpu(), logp.cpu(), mixed.cpu(), rep.cpu(), cur.cpu()


MIX_ROUTES = {"regs": (ROWS_V, ROWS_LD), "scalar": (5003, 5003), "vec": (10243, 10244)}


@pytest.mark.parametrize("p", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("route,k", [("regs", 0), ("regs", 5), ("regs", 1), ("scalar", 0), ("scalar", 5), ("vec", 0), ("vec", 5)])
def test_mix_rows_against_sample_rows(route, k, p):
    V, ld = MIX_ROUTES[route]
    if route == "regs":
        logits, u, _, _ = rows_inputs()
    else:
        logits, u, _ = route_inputs(V, ld)
    n = logits.shape[0]
    g = torch.Generator().manual_seed(n + k)
    coin = torch.rand(n, 2, generator=g)
    coin[0, 1], coin[1, 1] = 0.5, float(np.nextafter(np.float32(0.5), np.float32(0)))       # coin == p exactly; just below it
    teacher = torch.randint(0, V, (n, 4), generator=g)
    step = 3
    lens = torch.full((n,), 9, dtype=torch.int32)
    lens[2], lens[3], lens[4] = 3, 2, 4                       # the step is the row's last + 1 / beyond it: not valid; 4: valid
    inv_t = 1.0 if k != 5 else float(np.float32(1.0 / 0.7))
    fin = torch.zeros(n, dtype=torch.uint8)
    ids0, logp0, cur0, _ = _sample_rows(logits.cuda(), u.cuda(), fin.cuda(), inv_t, k, -1, V=V)
    ids, logp, mixed, rep, cur = _mix_rows(logits.cuda(), u.cuda(), coin.cuda(), p, teacher.cuda(), lens.cuda(), step, inv_t, k, V)
    want = torch.from_numpy((coin[:, 1].numpy() < np.float32(p)) & (step < lens.numpy()))
    assert want[0] == (p == 1.0) and want[1] == (p >= 0.5) and not want[2] and not want[3] and want[4] == (coin[4, 1].item() < p)
    if p == 0.0:
        assert not want.any()
    if p == 1.0:
        assert want.sum() == n - 2
    for x, fill in ((ids, -7), (mixed, -7), (rep, 9), (logp, 7.0)):                 # only column t is written
        assert (x[:, 0] == fill).all() and (x[:, 2] == fill).all()
    assert torch.equal(rep[:, 1].bool(), want) and ((rep[:, 1] == 0) | (rep[:, 1] == 1)).all()
    # replaced rows: st_sample_rows' token and logp, bit for bit
    assert torch.equal(mixed[:, 1][want], ids0[:, 1][want]) and torch.equal(ids[:, 1][want], ids0[:, 1][want])
    assert torch.equal(logp[:, 1][want].view(torch.int32), logp0[:, 1][want].view(torch.int32))
    # the others: the teacher's token, ids_out = -1, logp_out = 0
    assert torch.equal(mixed[:, 1][~want], teacher[:, 2][~want])
    assert (ids[:, 1][~want] == -1).all() and (logp[:, 1][~want] == 0).all()
    assert torch.equal(cur, mixed[:, 1])
    print(f"MEASURE mix rows {route} top_k {k} p {p}: replaced {int(want.sum())} of {n}")


def test_mix_rows_refuses_bad_arguments():
    from showtell_amd._lib import lib
    z = torch.zeros(4, 8, device="cuda")
    ids = torch.zeros(4, 4, device="cuda", dtype=torch.long)
    lens = torch.ones(4, device="cuda", dtype=torch.int32)
    rep = torch.zeros(4, 4, device="cuda", dtype=torch.uint8)
    cur = torch.zeros(4, device="cuda", dtype=torch.long)

    def call(p=0.5, t=1, k=0):
        return lib().st_sample_mix_rows(_ptr(z), 8, 4, 8, _ptr(z), 1, 1.0, k, _ptr(z), 1, p, _ptr(ids), 4, 0, _ptr(lens), 1, None, None,
                                        _ptr(ids), _ptr(rep), 4, t, _ptr(cur), _stream())
    assert call() == 0
    assert call(p=1.5) != 0 and b"outside [0, 1]" in lib().st_last_error()
    assert call(p=-0.5) != 0 and call(t=4) != 0 and call(k=33) != 0
    torch.cuda.synchronize()


# ====================================================================================================================
# 2: p = 1 against sample
# ====================================================================================================================

def _compare_with_sample(m, kind, feat, cap, lens, k, temperature):
    B, T = cap.shape
    u = torch.rand(2, B, T, generator=torch.Generator().manual_seed(77)).cuda()
    ids, rep = m.scheduled_inputs(feat, cap.cuda(), lens, 1.0, temperature, k, uniforms=u)
    valid = torch.from_numpy(K.valid_slots(kind, lens, T))
    assert torch.equal(rep.cpu(), valid)                      # p = 1: every valid slot
    if kind == "rnn":
        s_ids = m.sample(feat, 1, temperature, k, T, END, uniforms=u[1][:, None, :].contiguous())[0].view(B, T).cpu()
        mine = ids.cpu()
        slots = valid
    else:
        assert (cap[:, 0] == START).all()
        us = torch.cat([u[1][:, 1:], u[1][:, :1]], 1)          # sample's step t is the roll-in's slot t + 1
        s_ids = m.sample(feat, 1, temperature, k, T, START, END, uniforms=us[:, None, :].contiguous())[0].view(B, T).cpu()
        mine = torch.cat([ids.cpu()[:, 1:], torch.zeros(B, 1, dtype=torch.long)], 1)
        slots = torch.cat([valid[:, 1:], torch.zeros(B, 1, dtype=torch.bool)], 1)
        assert torch.equal(ids.cpu()[:, 0], cap[:, 0])        # <start> is never replaced
    e = (s_ids == END).long()
    upto = ((e.cumsum(1) - e) == 0) & slots                   # up to and including the first <end> or the last valid slot
    print(f"MEASURE p=1 against sample: {int(upto.sum())} of {int(slots.sum())} valid slots compared, rows that drew <end> early "
          f"{int(((e.cumsum(1) > 0) & slots).any(1).sum())}")
    assert upto.sum() >= slots[:, 0].sum() and upto.sum() > 0
    assert torch.equal(mine[upto], s_ids[upto])
    assert torch.equal(ids.cpu()[~valid], cap[~valid])


@pytest.mark.parametrize("case,k,temperature", [("gru777", 0, 1.0), ("lstm1500", 0, 0.8), ("gru_fp32", 5, 1.0), ("attn_fp32", 0, 1.0)])
def test_rate_one_is_sample(case, k, temperature):
    _, feat, cap, lens, _ = K.inputs(case)
    _compare_with_sample(_model(case, "rollin"), K.family(case), feat.cuda(), cap, lens, k, temperature)


def test_rate_one_is_sample_on_the_lstm_attention_decoder():
    from tests.test_gpu_attention import _make as make_attn
    params, feat, cap, lens = K.attn_lstm_inputs()
    m = make_attn("lstm", {k: v.clone() for k, v in params.items()}, torch.float32)
    _compare_with_sample(m, "attn", feat.cuda(), cap, lens, 0, 1.0)


# ====================================================================================================================
# 3: the float64 oracle walks the GPU's own mixed tokens
# ====================================================================================================================

@pytest.mark.parametrize("case", list(K.CASES))
def test_mixed_tokens_follow_the_storage_oracle(case):
    _, feat, cap, lens, _ = K.inputs(case)
    m = _model(case, "rollin")
    u = K.uniforms(case)
    ids, rep = m.scheduled_inputs(feat.cuda(), cap.cuda(), lens, K.P, uniforms=u.cuda())
    assert ids.dtype == torch.long and rep.dtype == torch.bool and ids.shape == rep.shape == cap.shape and ids.is_cuda
    ids, rep = ids.cpu(), rep.cpu()
    assert ((ids >= 0) & (ids < m.vocab_size)).all()
    want = torch.from_numpy(K.mix_rule(K.family(case), lens, u[0].numpy(), K.P))
    _, _, lp = K.roll_in(case, ids=ids)
    lo, hi = K.interval_excess(lp, ids, u[1])
    print(f"MEASURE {case}: replaced {int(rep.sum())} of {int(K.valid_slots(K.family(case), lens, cap.shape[1]).sum())} valid slots; "
          f"interval excess below {lo[want].max():.2e} above {hi[want].max():.2e} (d {K.d_bound(case):.2e})")
    assert torch.equal(rep, want)                             # (coin < p) & valid, exactly
    assert torch.equal(ids[~rep], cap[~rep])                  # the caption wherever nothing was replaced
    assert K.rollin_violations(case, ids, rep) == []


# ====================================================================================================================
# 4: loss(input_ids = X) against the float64 torch replica
# ====================================================================================================================

def _loss_run(case, m, variant, X, **extra):
    _, feat, cap, lens, alpha_c = K.inputs(case)
    kw = dict(extra)
    if variant == "w_ls":
        sw, tw = K.weights(case)
        kw.update(sequence_weight=sw.cuda(), token_weight=tw.cuda(), label_smoothing=K.LABEL_SMOOTHING[K.dtype_name(case)])
    for p in m.parameters():
        p.grad = None
    attn = K.family(case) == "attn"
    fd = feat.cuda().requires_grad_(not attn)
    args = (fd, cap.cuda(), lens) + ((alpha_c,) if attn else ())
    loss = m.loss(*args, input_ids=None if X is None else X.cuda(), **kw)
    loss.backward()
    torch.cuda.synchronize()
    g = {k: p.grad.detach().float().cpu() for k, p in m.named_parameters()}
    if not attn:
        g["feat"] = fd.grad.detach().float().cpu()
    return loss.item(), g


def _check_loss(case, variant, loss, g, tag):
    ref = K.loss_reference(case, variant)
    bound = K.loss_bound(case, ref)
    print(f"MEASURE {tag}: loss {loss:.6f} oracle {ref['loss']:.6f} |d| {abs(loss - ref['loss']):.2e} (bound {bound:.2e})")
    K.assert_grads_within_linear_bound(g, ref, K.GRAD_TOL[K.dtype_name(case)], tag)
    assert abs(loss - ref["loss"]) <= bound
    only = K.target_only_tokens(case)
    assert len(only) >= 2
    assert (g["embeddings.weight"][only] == 0).all(), "an embedding row that was never fed has a gradient"


@pytest.mark.parametrize("variant", ["plain", "w_ls"])
@pytest.mark.parametrize("case,fused", K.ROUTES)
def test_loss_with_input_ids_matches_the_float64_replica(case, fused, variant, monkeypatch):
    monkeypatch.setenv("ST_FUSED_CE", fused)
    m = _model(case, "loss")
    loss, g = _loss_run(case, m, variant, K.random_ids(case))
    _check_loss(case, variant, loss, g, f"{case} ST_FUSED_CE={fused} {variant}")


@pytest.mark.parametrize("fused", ["1", "0"])
def test_loss_with_input_ids_and_dropout_matches_the_float64_replica(fused, monkeypatch):
    from showtell_amd.rnn import RNN
    monkeypatch.setenv("ST_FUSED_CE", fused)
    case = "gru777"
    _, cell, _, E, H, V, L, _ = K.CASES[case]
    p_in, p_layer, p_out = K.DROPOUT["p"]
    m = RNN(E, H, V, L, dtype=K.torch_dtype(case), dropout=p_layer, dropout_in=p_in, dropout_out=p_out)
    m.load_state_dict({k: v.clone() for k, v in K.inputs(case)[0].items()})
    m = m.cuda().train()
    m.seed_dropout(K.DROPOUT["seed"])                         # the call below draws step 0 of the masks
    loss, g = _loss_run(case, m, "dropout", K.random_ids(case))
    _check_loss(case, "dropout", loss, g, f"{case} ST_FUSED_CE={fused} dropout")


@pytest.mark.parametrize("case", ["gru777", "attn_fp32"])
def test_forward_and_token_logp_take_input_ids(case):
    """forward(input_ids = X) gives the logits whose cross entropy against the caption is loss(input_ids = X), and token_logp(..,
    input_ids = X) sums to it."""
    _, feat, cap, lens, alpha_c = K.inputs(case)
    m = _model(case, "loss")
    X = K.random_ids(case).cuda()
    attn = K.family(case) == "attn"
    ref = K.loss_reference(case, "plain")
    with torch.no_grad():
        out = m(feat.cuda(), cap.cuda(), lens, input_ids=X)
        logits = out[0] if attn else out
        lp = m.token_logp(feat.cuda(), cap.cuda(), lens, input_ids=X)
    from oracle import restatement as R
    ce = torch.nn.functional.cross_entropy(logits.double().cpu(), R.pack_rows(cap, lens)).item()
    want = ref["loss"]
    if attn:                                                  # the oracle's loss holds the doubly-stochastic term too
        want -= alpha_c * ((1.0 - out[1].double().cpu().sum(dim=1)) ** 2).mean().item()
    nll = -lp.double().sum().item() / sum(lens)
    print(f"MEASURE {case}: CE(forward(input_ids)) {ce:.6f}, -sum token_logp / N {nll:.6f}, oracle {want:.6f}")
    assert abs(ce - want) <= K.loss_bound(case, ref) and abs(nll - want) <= K.loss_bound(case, ref)
    assert (lp.cpu()[~torch.from_numpy(np.arange(cap.shape[1])[None, :] < np.asarray(lens)[:, None])] == 0).all()


# ====================================================================================================================
# 5: None and the caption itself
# ====================================================================================================================

ROLL_IN_ENTRY_POINTS = ("st_rnn_sched_inputs", "st_attn_sched_inputs", "st_sample_mix_rows")
TAKES_INPUT_IDS = (("st_rnn_forward", 11), ("st_rnn_backward", 9))      # entry point, index of its input_ids argument


@pytest.mark.parametrize("case,fused", [("gru777", "1"), ("gru777", "0"), ("gru_fp32", "1"), ("attn_fp32", "1")])
def test_none_is_the_call_it_was_and_the_caption_is_the_plain_loss(case, fused, monkeypatch):
    from showtell_amd._lib import lib
    monkeypatch.setenv("ST_FUSED_CE", fused)
    _, feat, cap, lens, _ = K.inputs(case)
    m = _model(case, "loss").eval()
    try:
        def refuse(*a):
            raise AssertionError("input_ids=None reached a scheduled-sampling entry point")

        def refuse_ids(real, i):                              # the call itself goes through; a non-NULL input_ids does not
            return lambda *a: refuse() if a[i] is not None else real(*a)
        loss0, g0 = _loss_run(case, m, "plain", None)
        with monkeypatch.context() as mp:
            for name in ROLL_IN_ENTRY_POINTS:
                mp.setattr(lib(), name, refuse)
            for name, i in TAKES_INPUT_IDS:
                mp.setattr(lib(), name, refuse_ids(getattr(lib(), name), i))
            loss1, g1 = _loss_run(case, m, "plain", None)
            loss2, _ = _loss_run(case, m, "plain", None, scheduled_sampling=0.0)      # p = 0 runs no roll-in at all
            with torch.no_grad():
                out0 = m(feat.cuda(), cap.cuda(), lens)
                m.token_logp(feat.cuda(), cap.cuda(), lens)
            with pytest.raises(AssertionError, match="reached a scheduled-sampling entry point"):
                _loss_run(case, m, "plain", None, scheduled_sampling=0.5)           # the patch is in the way of the roll-in
            if K.family(case) != "attn":
                with pytest.raises(AssertionError, match="reached a scheduled-sampling entry point"):
                    _loss_run(case, m, "plain", cap)
        loss3, g3 = _loss_run(case, m, "plain", cap)
        with torch.no_grad():
            out3 = m(feat.cuda(), cap.cuda(), lens, input_ids=cap.cuda())
        print(f"MEASURE {case} ST_FUSED_CE={fused}: plain {loss0!r}, None again {loss1!r}, p=0 {loss2!r}, input_ids=cap {loss3!r}")
        for other in (loss1, loss2, loss3):
            assert abs(other - loss0) <= 1e-6 * abs(loss0)
        a, b = (out0[0], out3[0]) if K.family(case) == "attn" else (out0, out3)
        assert torch.equal(a, b)                              # the plain logits, bit for bit
        for k in g0:
            scale = g0[k].abs().max().item() + 1e-30
            assert (g3[k] - g0[k]).abs().max().item() <= 1e-6 * scale, k     # the order of the fp32 atomics only
    finally:
        m.train()


# ====================================================================================================================
# 6: determinism; nothing allocated, nothing synchronised
# ====================================================================================================================

@pytest.mark.parametrize("case", ["gru777", "attn_fp32"])
def test_same_seed_or_same_uniforms_give_the_same_tensors(case):
    _, feat, cap, lens, _ = K.inputs(case)
    m = _model(case, "rollin")
    f, c = feat.cuda(), cap.cuda()
    outs = []
    for _ in range(2):
        g = torch.Generator(device="cuda")
        g.manual_seed(5)
        outs.append(m.scheduled_inputs(f, c, lens, 0.5, temperature=0.9, top_k=20, generator=g))
    u = K.uniforms(case).cuda()
    outs += [m.scheduled_inputs(f, c, lens, 0.5, uniforms=u) for _ in range(2)]
    for a, b in ((outs[0], outs[1]), (outs[2], outs[3])):
        assert len(a) == 2 and all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(outs[0][1], outs[2][1])            # other coins, other slots
    ids0, rep0 = m.scheduled_inputs(f, c, lens, 0.0, uniforms=u)
    assert torch.equal(ids0, c) and not rep0.any()


def test_rnn_sched_inputs_allocates_and_synchronises_nothing():
    """st_rnn_sched_inputs on a side stream with preallocated buffers, recorded into a graph: a capture admits neither an
    allocation nor a synchronisation, and its replay gives the eager call's tensors."""
    from showtell_amd._lib import check, lib
    case = "gru777"
    _, feat, cap, lens, _ = K.inputs(case)
    m = _model(case, "rollin")
    prm, keep = m._c_params()
    B, T = cap.shape
    featd = feat.cuda().bfloat16()
    capd = cap.cuda().contiguous()
    lensd = torch.tensor(lens, dtype=torch.int32).cuda()
    u = K.uniforms(case).cuda()
    nbytes = lib().st_rnn_sched_inputs_workspace_bytes(C.byref(prm), B)
    ws = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
    ids = torch.empty(B, T, device="cuda", dtype=torch.long)
    rep = torch.empty(B, T, device="cuda", dtype=torch.uint8)
    drawn = torch.empty(B, T, device="cuda", dtype=torch.long)
    logp = torch.empty(B, T, device="cuda")
    s = torch.cuda.Stream()

    def call():
        check(lib().st_rnn_sched_inputs(C.byref(prm), _ptr(featd), B, _ptr(capd), T, _ptr(lensd), max(lens), _ptr(u[0]), _ptr(u[1]), K.P, 1.0,
                                        0, _ptr(ws), nbytes, _ptr(ids), _ptr(rep), _ptr(drawn), _ptr(logp), _stream()), "st_rnn_sched_inputs")
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    s.synchronize()
    eager = [x.clone() for x in (ids, rep, drawn, logp)]
    for x in (ids, rep, drawn, logp):
        x.fill_(3)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip((ids, rep, drawn, logp), eager))
    # and it is what the Python call returns; drawn / logp are the documented optional outputs
    pid, prep = m.scheduled_inputs(feat.cuda(), capd, lens, K.P, uniforms=u)
    assert torch.equal(pid, ids) and torch.equal(prep, rep.bool())
    r = rep.bool()
    assert torch.equal(drawn[r], ids[r]) and (drawn[~r] == -1).all() and (logp[~r] == 0).all() and (logp[r] <= 0).all()


# ====================================================================================================================
# 7: the Trainer
# ====================================================================================================================

def _training_pair():
    from oracle import restatement as R
    from showtell_amd import optim
    from showtell_amd.cnn import ResNet
    from showtell_amd.rnn import RNN
    from showtell_amd.train import Trainer
    E, H, V, L, B = 64, 64, 120, 2, 4
    enc = R.init_encoder_params(18, E, seed=2)
    dec = R.init_decoder_params(E, H, V, L, "gru", seed=2)
    # The head's BatchNorm bias starts at exactly 0 in the seeded parameters: after two steps such a parameter IS its accumulated
    # updates, and "relative to the parameter" then measures the gradient's own atomics noise (8 ulp of fp32 a step,
    # tests/test_gpu_dropout.py ATOMIC_REL, compounding over two momentum steps; 2.3e-6 measured on an MI355X), not the agreement
    # of the two sequences.  It gets a scale of its own, as every other trainable parameter has.
    enc["last_layer.bias"] = 0.1 * torch.randn(E, generator=torch.Generator().manual_seed(7))
    cnn = ResNet(18, E); cnn.load_state_dict(enc); cnn = cnn.cuda().train()
    rnn = RNN(E, H, V, L); rnn.load_state_dict(dec); rnn = rnn.cuda().train()
    opt = optim.SGD(Trainer.trainable_params(cnn, rnn), lr=0.05, momentum=0.9)
    return cnn, rnn, opt


def test_trainer_step_is_the_manual_sequence():
    from oracle import restatement as R
    from showtell_amd.train import Trainer
    cap, lens = R.synthetic_captions(4, 120, seed=2, mean=6, std=1.5, lo=4, hi=9)
    imgs = [torch.randn(4, 3, 96, 96, generator=torch.Generator().manual_seed(s)).cuda() for s in (2, 3)]
    capd = cap.cuda()
    # the Trainer
    cnn, rnn, opt = _training_pair()
    g = torch.Generator(device="cuda"); g.manual_seed(11)
    tr = Trainer(cnn, rnn, opt, scheduled_sampling=0.5, ss_generator=g)
    losses = [tr.step(im, capd, lens).item() for im in imgs]
    tr.flush()
    # by hand: the same features (a Trainer without scheduled sampling prepares them), then scheduled_inputs + loss(input_ids=)
    cnn2, rnn2, opt2 = _training_pair()
    g2 = torch.Generator(device="cuda"); g2.manual_seed(11)
    tr2 = Trainer(cnn2, rnn2, opt2)
    losses2, replaced = [], 0
    for im in imgs:
        feat = tr2._features(im, ())
        ids, rep = rnn2.scheduled_inputs(feat, capd, lens, 0.5, generator=g2)
        replaced += int(rep.sum())
        loss = rnn2.loss(feat, capd, lens, input_ids=ids)
        loss.backward()
        opt2.step()
        losses2.append(loss.item())
    torch.cuda.synchronize()
    assert replaced > 0
    worst, where = 0.0, None
    for (k, a), (_, b) in zip(list(rnn.named_parameters()) + list(cnn.named_parameters()), list(rnn2.named_parameters()) + list(cnn2.named_parameters())):
        d = ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()
        if d > worst:
            worst, where = d, k
    print(f"MEASURE trainer: losses {losses} by hand {losses2}; replaced slots {replaced}; parameters differ by at most {worst:.2e} relative "
          f"({where})")
    assert all(abs(a - b) <= 1e-6 * abs(b) for a, b in zip(losses, losses2))
    assert worst <= 1e-6
    # and the mixed inputs matter: the plain step lands elsewhere
    cnn3, rnn3, opt3 = _training_pair()
    tr3 = Trainer(cnn3, rnn3, opt3)
    l3 = [tr3.step(im, capd, lens).item() for im in imgs]
    assert abs(l3[0] - losses[0]) > 1e-4 * abs(l3[0])


def test_trainer_asks_a_callable_schedule_with_the_step_count():
    from oracle import restatement as R
    from showtell_amd.train import Trainer
    cap, lens = R.synthetic_captions(4, 120, seed=2, mean=6, std=1.5, lo=4, hi=9)
    im = torch.randn(4, 3, 96, 96, generator=torch.Generator().manual_seed(2)).cuda()
    cnn, rnn, opt = _training_pair()
    asked = []

    def schedule(i):
        asked.append(i)
        return 0.0 if i == 0 else 1.0
    tr = Trainer(cnn, rnn, opt, scheduled_sampling=schedule)
    for _ in range(3):
        tr.step(im, cap.cuda(), lens)
    tr.flush()
    assert asked == [0, 1, 2]
    with pytest.raises(ValueError):
        Trainer(cnn, rnn, opt, scheduled_sampling=lambda i: 2.0).step(im, cap.cuda(), lens)
