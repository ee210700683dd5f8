"""Per-token loss weights, token_logp and the self-critical step on the GPU (csrc/vocab_ce.hip, the st_cross_entropy kernels,
rnn.loss / token_logp, Trainer.step_self_critical).  The cases, the signed weights and the float64 oracle come from
tests/_weighted_loss_cases.py; tests/test_weighted_loss_inputs.py shows from the oracle alone that the gradient bound has power.

Shapes: E = H = 512, L = 2 with (gru, V = 777, B = 9) and (lstm, V = 1500, B = 33) -- V no multiple of the 128-entry tile, the
token count no multiple of the 32-token tile, B = 33 more than one 64-token block of the reduction -- on the fused route and on
ST_FUSED_CE=0; an fp32 decoder at E = H = 64, V = 200 and the fp32 attention fixture for st_cross_entropy with row weights."""
import ctypes as C

import pytest
import torch

from oracle import restatement as R
from tests import _weighted_loss_cases as W

pytestmark = pytest.mark.gpu

# (case, ST_FUSED_CE): the bf16 H = 512 cases run both routes; the others have only the launch chain
ROUTES = [("gru777", "1"), ("gru777", "0"), ("lstm1500", "1"), ("lstm1500", "0"), ("gru_fp32", "1"), ("attn_fp32", "1")]
LIN_WEIGHTS = (0.0, 0.5, -0.5, 1.0, -1.0, 2.0, 4.0)          # powers of two commute with the bf16 rounding of dlogits

# token_logp against log_softmax (float64) of forward()'s fp32 logits: 4 x the largest difference measured on an MI355X at these
# shapes (the fp32 summation order of the K = H product and the fast exp / log), never more than 5e-3; a wrong row or target is O(1)
LOGP_MEASURED = {("gru777", "1"): 1.277e-6, ("gru777", "0"): 1.163e-6, ("lstm1500", "1"): 1.418e-6, ("lstm1500", "0"): 1.418e-6,
                 ("gru_fp32", "1"): 8.116e-7, ("attn_fp32", "1"): 5.265e-7}


def _model(case):
    from tests.test_gpu_attention import _make as make_attn
    from tests.test_gpu_decoder import _make_sized
    family, cell, _, E, H, V, L, _ = W.CASES[case]
    params = W.inputs(case)[0]
    if family == "attn":
        return make_attn(cell, {k: v.clone() for k, v in params.items()}, torch.float32).train()
    return _make_sized(cell, params, W.torch_dtype(case), E, H, V, L)


def _loss(case, m, feat, cap, lens, alpha_c, **kw):
    if W.CASES[case][0] == "attn":
        return m.loss(feat, cap, lens, alpha_c, **kw)
    return m.loss(feat, cap, lens, **kw)


def _run(case, m, **kw):
    """loss and every gradient of one loss() + backward on the case's inputs."""
    _, feat, cap, lens, alpha_c = W.inputs(case)
    for p in m.parameters():
        p.grad = None
    fd = feat.cuda().requires_grad_(True)
    loss = _loss(case, m, fd, cap.cuda(), lens, alpha_c, **kw)
    loss.backward()
    torch.cuda.synchronize()
    g = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    if W.CASES[case][0] != "attn":             # the attention decoder's feature map comes from a frozen backbone: no gradient
        g["feat"] = fd.grad.detach().clone()
    return loss.item(), g


def _lin_weights(n):
    idx = torch.randint(0, len(LIN_WEIGHTS), (n,), generator=torch.Generator().manual_seed(23))
    idx[:len(LIN_WEIGHTS)] = torch.arange(len(LIN_WEIGHTS))       # every value occurs
    return torch.tensor(LIN_WEIGHTS)[idx]


def _check_linear(d1, dw, w, V, nll, loss1, lossw):
    n = d1.shape[0]
    d1f, dwf = d1.float(), dw.float()
    assert d1f[:, :V].abs().max().item() > 0 and torch.isfinite(d1f).all()
    assert torch.equal(dwf, w[:, None] * d1f)                     # elementwise, every row, pad columns included
    assert (dwf[w == 0] == 0).all() and (dwf[:, V:] == 0).all() and (d1f[:, V:] == 0).all()
    assert (dwf[w != 0][:, :V] != 0).any(1).all()
    nll64 = nll.double()
    assert (nll64 > 0).all()
    assert abs(loss1.item() - nll64.mean().item()) <= 1e-5 * nll64.mean().item()
    assert abs(lossw.item() - (w.double() * nll64).sum().item() / n) <= 1e-5 * (w.double().abs() * nll64).sum().item() / n


@pytest.mark.parametrize("case,fused", ROUTES)
def test_dlogits_are_linear_in_the_row_weight_bit_for_bit(case, fused):
    """The C entry points directly: dlogits_w[r] == w_r * dlogits_1[r] elementwise, dlogits_1 from the call with NULL
    terms (weights from {0, +-0.5, +-1, 2, 4}); zero-weight rows and pad columns all zero; nll_out and the weighted sum agree
    with the unweighted loss.  Catches a wrong packed-row index, a weight applied to pad columns, a missed tile."""
    from showtell_amd._lib import check, dtype_code, lib
    from showtell_amd.rnn import _cp, _stream, loss_terms, up8
    from showtell_amd.seq import plan_for
    family = W.CASES[case][0]
    _, feat, cap, lens, _ = W.inputs(case)
    m = _model(case)
    dt, V = m.compute_dtype, m.vocab_size
    capd = cap.cuda().contiguous()
    n = sum(lens)
    w = _lin_weights(n).cuda()
    gsc = torch.full((), 0.75, device="cuda")
    loss1, lossw = torch.zeros((), device="cuda"), torch.zeros((), device="cuda")
    nll = torch.full((n,), -1.0, device="cuda")
    terms = loss_terms(w, nll)                                    # plain calls: NULL terms; weighted ones: row_weight and nll_out
    if family == "attn":
        with torch.no_grad():
            logits = m(feat.cuda(), capd, lens)[0].contiguous()
        targets = R.pack_rows(cap, lens).cuda()
        ldl, ldd, ldt = V, up8(V), torch.float32
    else:
        plan = plan_for(lens, torch.device("cuda", torch.cuda.current_device()))
        seq = plan.c_struct(capd)
        prm, keep = m._c_params()
        nbytes = lib().st_rnn_workspace_bytes(C.byref(prm), C.byref(seq))
        ws = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
        targets = torch.empty(n, device="cuda", dtype=torch.long)
        ldl = ldd = lib().st_rnn_vocab_ld(V)
        ldt = dt
        use_fused = fused == "1" and bool(lib().st_rnn_fused_loss_supported(C.byref(prm)))
        assert use_fused == (fused == "1" and dt == torch.bfloat16)
        logits = None if use_fused else torch.empty(n, ldl, device="cuda", dtype=ldt)
        check(lib().st_rnn_forward(C.byref(prm), C.byref(seq), _cp(m._feature(feat.cuda())), _cp(ws), nbytes, _cp(logits),
                                   dtype_code(ldt), ldl, _cp(targets), 1, None, None, _stream()), "st_rnn_forward")
        if use_fused:
            sb = lib().st_rnn_fused_loss_bytes(C.byref(prm), C.byref(seq))
            s1, sw_ = (torch.empty(sb // 4, device="cuda") for _ in range(2))
            d1, dw = (torch.full((n, ldd), 7.0, device="cuda", dtype=dt) for _ in range(2))
            a = (C.byref(prm), C.byref(seq), _cp(ws), nbytes, _cp(targets))
            check(lib().st_rnn_fused_loss(*a, _cp(s1), sb, None, _cp(loss1), None, _stream()), "st_rnn_fused_loss")
            check(lib().st_rnn_fused_dlogits(*a, _cp(s1), _cp(gsc), None, _cp(d1), ldd, None, _stream()), "st_rnn_fused_dlogits")
            check(lib().st_rnn_fused_loss(*a, _cp(sw_), sb, C.byref(terms), _cp(lossw), None, _stream()), "st_rnn_fused_loss")
            check(lib().st_rnn_fused_dlogits(*a, _cp(sw_), _cp(gsc), C.byref(terms), _cp(dw), ldd, None, _stream()), "st_rnn_fused_dlogits")
            torch.cuda.synchronize()
            assert torch.equal(s1[:n], sw_[:n])                   # the rows' logsumexp does not depend on the weights
            _check_linear(d1, dw, w, V, nll, loss1, lossw)
            return
    d1, dw = (torch.full((n, ldd), 7.0, device="cuda", dtype=ldt) for _ in range(2))
    dtc = dtype_code(ldt)
    check(lib().st_cross_entropy(_cp(logits), dtc, _cp(targets), n, V, ldl, None, _cp(loss1), _cp(d1), dtc, ldd, 1.0, _cp(gsc), _stream()),
          "st_cross_entropy")
    check(lib().st_cross_entropy(_cp(logits), dtc, _cp(targets), n, V, ldl, C.byref(terms), _cp(lossw), _cp(dw), dtc, ldd, 1.0, _cp(gsc),
                                 _stream()), "st_cross_entropy")
    torch.cuda.synchronize()
    _check_linear(d1, dw, w, V, nll, loss1, lossw)


@pytest.mark.parametrize("case,fused", ROUTES)
def test_weighted_loss_and_gradients_match_the_float64_oracle(case, fused, monkeypatch):
    """Signed weights per sequence and per token (they multiply).  Every parameter's gradient and the feature's:
    max|g_gpu(w) - g_ref(w)| <= tol * (max|g_ref(w+)| + max|g_ref(w-)|), tol 4e-2 (bf16) / 1e-3 (fp32); the loss to 2e-2 * mean|w|
    (bf16).  fp32 loss: 1e-4 * mean|w|, the bound of test_fp32_full_size_gru_step_matches_oracle in the same linear form, plus
    for the attention decoder the 3e-5 that tests/test_gpu_attention.py allows its (here unweighted) loss."""
    monkeypatch.setenv("ST_FUSED_CE", fused)
    sw, tw = W.weights(case)
    ref = W.reference(case)
    m = _model(case)
    loss, g = _run(case, m, sequence_weight=sw.cuda(), token_weight=tw)        # one weight on the device, one on the host
    dt = W.CASES[case][2]
    mean_w = W.packed_weights(case).abs().mean().item()
    bound = 2e-2 * mean_w if dt == "bf16" else 1e-4 * mean_w + (3e-5 if W.CASES[case][0] == "attn" else 0.0)
    print(f"MEASURE {case} fused={fused}: loss {loss:.6f} oracle {ref['loss']:.6f} diff {abs(loss - ref['loss']):.3e} bound {bound:.3e}")
    assert set(g) == set(ref["g"])
    W.assert_grads_within_linear_bound(g, ref, W.GRAD_TOL[dt], f"MEASURE {case} fused={fused}")
    assert abs(loss - ref["loss"]) <= bound
    # either weight alone, against both: the same rows through the other argument
    _, _, cap, lens, _ = W.inputs(case)
    both = (sw[:, None] * tw).cuda()
    loss_t, g_t = _run(case, m, token_weight=both)
    assert abs(loss_t - loss) <= 1e-6 * abs(loss) + 1e-9
    for k in g:
        assert (g_t[k] - g[k]).abs().max().item() <= 1e-6 * g[k].abs().max().item() + 1e-12, k


@pytest.mark.parametrize("case,fused", ROUTES)
def test_token_logp_matches_log_softmax_of_the_forward_logits(case, fused, monkeypatch):
    """token_logp against log_softmax in float64 of the fp32 logits the unchanged forward() returns, at the targets.
    Largest difference measured on an MI355X: gru777 fused 1.277e-06, chain 1.163e-06; lstm1500 fused 1.418e-06, chain 1.418e-06;
    gru_fp32 8.116e-07; attn_fp32 5.265e-07 -- two to three units in the last place of an fp32 log-probability near -7 (bound:
    4 x the measurement, at most 5e-3).
    -token_logp.sum() / N_tok equals loss() to 1e-5 relative (not asked of ST_FUSED_CE=0 in bf16, where loss() rounds the logits
    it hands to st_cross_entropy to bf16 and token_logp keeps them fp32); entries past lens[b] are exactly 0."""
    monkeypatch.setenv("ST_FUSED_CE", fused)
    family = W.CASES[case][0]
    _, feat, cap, lens, _ = W.inputs(case)
    m = _model(case)
    wide = torch.cat([cap, torch.zeros(cap.shape[0], 2, dtype=torch.long)], 1).cuda()      # a caption tensor wider than lens[0]
    with torch.no_grad():
        out = m(feat.cuda(), cap.cuda(), lens)
        logits = (out[0] if family == "attn" else out).double().cpu()
        lp = m.token_logp(feat.cuda(), wide, lens)
        plain = _loss(case, m, feat.cuda(), cap.cuda(), lens, 0.0).item()
    torch.cuda.synchronize()
    assert lp.shape == tuple(wide.shape) and lp.dtype == torch.float32 and not lp.requires_grad
    target = R.pack_rows(cap, lens)
    ref = torch.log_softmax(logits, 1).gather(1, target[:, None])[:, 0]
    lpc = lp.cpu()
    diff = (R.pack_rows(lpc, lens).double() - ref).abs().max().item()
    bound = min(4 * LOGP_MEASURED[(case, fused)], 5e-3)
    print(f"MEASURE token_logp {case} fused={fused}: max diff {diff:.3e} (bound {bound:.3e}); loss {plain:.6f} "
          f"-sum/ntok {-lpc.double().sum().item() / len(target):.6f}")
    for b, l in enumerate(lens):
        assert (lpc[b, l:] == 0).all() and (lpc[b, :l] < 0).all()
    assert diff <= bound
    if not (fused == "0" and W.CASES[case][2] == "bf16"):
        assert abs(-lpc.double().sum().item() / len(target) - plain) <= 1e-5 * abs(plain)


@pytest.mark.parametrize("case,fused", ROUTES)
def test_weights_of_one_give_the_plain_loss(case, fused, monkeypatch):
    """sequence_weight = ones against no weights: loss and gradients to 1e-6 relative (the order of the fp32 atomics only)."""
    monkeypatch.setenv("ST_FUSED_CE", fused)
    m = _model(case)
    B = W.inputs(case)[2].shape[0]
    loss0, g0 = _run(case, m)
    loss1, g1 = _run(case, m, sequence_weight=torch.ones(B))
    assert abs(loss1 - loss0) <= 1e-6 * abs(loss0)
    for k in g0:
        assert (g1[k] - g0[k]).abs().max().item() <= 1e-6 * g0[k].abs().max().item(), k


# ---- Trainer.step_self_critical: ResNet-18 at 64 x 64, B = 4 images, S = 3 samples each ---------------------------------------
SC = dict(E=64, H=64, V=120, L=2, B=4, S=3, seed=2)
HEAD = ("linear_secondlast_layer.weight", "linear_secondlast_layer.bias", "last_layer.weight", "last_layer.bias")


def _sc_setup():
    from showtell_amd import optim
    from showtell_amd.cnn import ResNet
    from showtell_amd.rnn import RNN
    from showtell_amd.train import Trainer
    c = SC
    enc = R.init_encoder_params(18, c["E"], seed=c["seed"])
    dec = R.init_decoder_params(c["E"], c["H"], c["V"], c["L"], "gru", seed=c["seed"])
    dec["linear.bias"][2] += 3.0               # <end> likely enough that the 12 samples end at different steps
    cnn = ResNet(18, c["E"]); cnn.load_state_dict(enc); cnn = cnn.cuda().train()
    rnn = RNN(c["E"], c["H"], c["V"], c["L"]); rnn.load_state_dict(dec); rnn = rnn.cuda().train()
    img = torch.randn(c["B"], 3, 64, 64, generator=torch.Generator().manual_seed(c["seed"]))
    opt = optim.SGD(Trainer.trainable_params(cnn, rnn), lr=0.1, momentum=0.0)
    return enc, dec, cnn, rnn, img, Trainer(cnn, rnn, opt)


def _sc_reward(ids, lengths):
    """A fixed, non-constant function of the sampled ids."""
    pos = torch.arange(1, ids.shape[-1] + 1)
    return ((ids * pos).sum(-1) % 11).float() / 10.0 + 0.05 * lengths.float()


def test_self_critical_step_with_a_constant_reward_changes_no_parameter():
    """The advantage is 0: after an SGD step without momentum every parameter is bit for bit what it was."""
    _, _, cnn, rnn, img, tr = _sc_setup()
    params = tr.trainable_params(cnn, rnn)
    before = [p.detach().clone() for p in params]
    seen = []

    def reward_fn(ids, lengths):
        seen.append((tuple(ids.shape), tuple(lengths.shape), ids.device.type))
        return torch.full(tuple(lengths.shape), 0.7)
    loss, mean_reward = tr.step_self_critical(img.cuda(), reward_fn, num_samples=SC["S"], generator=torch.Generator().manual_seed(7))
    tr.flush()
    torch.cuda.synchronize()
    assert seen == [((SC["B"], 1, 25), (SC["B"], 1), "cpu"), ((SC["B"], SC["S"], 25), (SC["B"], SC["S"]), "cpu")]   # greedy, then the samples
    assert loss.item() == 0.0 and abs(float(mean_reward) - 0.7) < 1e-6
    for p, b in zip(params, before):
        assert torch.equal(p.detach(), b)
    # baseline='mean' as well
    loss, _ = tr.step_self_critical(img.cuda(), reward_fn, num_samples=SC["S"], baseline="mean", generator=torch.Generator().manual_seed(8))
    tr.flush()
    assert loss.item() == 0.0
    for p, b in zip(params, before):
        assert torch.equal(p.detach(), b)


@pytest.mark.parametrize("baseline", ["greedy", "mean"])
def test_self_critical_step_gradients_match_the_oracle_on_the_sampled_ids(baseline):
    """A fixed non-constant reward, against the greedy caption's reward and against the mean of the image's other samples (there
    the advantages have both signs whatever the reward).  The oracle (float64: R.encoder_forward, R.rnn_forward, the weighted loss of
    tests/_weighted_loss_cases.py) is fed the GPU's own sampled ids; decoder and head gradients obey the linear-form bound at
    1e-3 (fp32).  d(loss)/d(linear_secondlast_layer.bias) is analytically zero under batch-statistics BatchNorm: held to the
    absolute 1e-4 of test_encoder_head_linear_bn1d."""
    from showtell_amd.train import sample_caption_batch, self_critical_advantage
    enc, dec, cnn, rnn, img, tr = _sc_setup()
    B, S = SC["B"], SC["S"]
    calls = []

    def reward_fn(ids, lengths):
        calls.append((ids.clone(), lengths.clone()))
        return _sc_reward(ids, lengths)
    loss, mean_reward = tr.step_self_critical(img.cuda(), reward_fn, num_samples=S, baseline=baseline,
                                              generator=torch.Generator().manual_seed(7))
    torch.cuda.synchronize()
    got = {k: p.grad.detach().clone() for k, p in rnn.named_parameters()}
    got.update({k: dict(cnn.named_parameters())[k].grad.detach().clone() for k in HEAD})
    assert len(calls) == (2 if baseline == "greedy" else 1)                 # the greedy row is scored only where it is the baseline
    ids, lengths = calls[-1]
    reward = _sc_reward(ids, lengths)
    adv = self_critical_advantage(reward, baseline, _sc_reward(*calls[0]) if baseline == "greedy" else None)
    assert (adv != 0).sum() >= B * S // 2 and len(set(lengths.reshape(-1).tolist())) >= 3           # weights that matter, ragged rows
    if baseline == "mean":
        assert (adv > 0).any() and (adv < 0).any()
    assert abs(float(mean_reward) - reward.mean().item()) < 1e-6
    order, cap, lens = sample_caption_batch(ids, lengths)
    # oracle
    po = {k: v.double().clone() for k, v in enc.items()}
    for k in HEAD:
        po[k].requires_grad_(True)
    do = {k: v.double().clone().requires_grad_(True) for k, v in dec.items()}
    feat = R.encoder_forward(po, img.double(), 18, train=True)[order // S]
    logits = R.rnn_forward(do, feat, cap, lens)
    w = R.pack_rows(adv.double().reshape(-1)[order][:, None].expand(B * S, cap.shape[1]), lens)
    leaves = {**do, **{k: po[k] for k in HEAD}}
    ref = {}
    for name, wk in (("g", w), ("gp", w.clamp(min=0)), ("gm", (-w).clamp(min=0))):
        lo = W.weighted_loss(logits, None, R.pack_rows(cap, lens), wk, 0.0)
        ref[name] = dict(zip(leaves, torch.autograd.grad(lo, list(leaves.values()), retain_graph=True)))
        if name == "g":
            ref["loss"] = lo.item()
    print(f"MEASURE self-critical: loss {loss.item():.6f} oracle {ref['loss']:.6f}; lens {lens}")
    zero = got.pop("linear_secondlast_layer.bias")
    assert zero.abs().max().item() < 1e-4
    W.assert_grads_within_linear_bound(got, ref, W.GRAD_TOL["fp32"], "MEASURE self-critical")
    assert abs(loss.item() - ref["loss"]) <= 1e-4 * w.abs().mean().item()
    tr.flush()
