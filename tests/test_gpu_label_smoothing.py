"""Label smoothing on the GPU: the LS instantiations of csrc/vocab_ce.hip (fused bf16 route) and of ce_kernel (the bf16 and fp32
launch chains, both attention decoders), the C entry points st_rnn_fused_loss / st_rnn_fused_dlogits / st_cross_entropy with
smoothing = 1 in their st_loss_terms, rnn.loss(.., label_smoothing=) and Trainer(.., label_smoothing=).  Cases, float64 oracle
(torch's F.cross_entropy(label_smoothing=) on the logits of oracle/restatement.py) and bounds come from tests/_label_smoothing_cases.py;
tests/test_label_smoothing_inputs.py shows on the CPU that these inputs and bounds catch the faults they are meant to catch.

Shapes: E = H = 512 with (gru, V = 777, 66 tokens = two token tiles + 2 rows), (lstm, V = 1500, more than two 64-token blocks of
the reduction) and (gru, V = 130, L = 1: a second entry tile with 2 valid entries and three masked waves) on the fused route,
V = 777 also on ST_FUSED_CE=0; an fp32 decoder at E = H = 64, V = 200 and the fp32 attention fixture on the launch chain.

Measured on an MI355X (max over rows |smooth_out - u64|, bound 4 x the CPU floor): see DESIGN.md section 7."""
import ctypes as C

import pytest
import torch

from oracle import restatement as R
from tests import _label_smoothing_cases as S

pytestmark = pytest.mark.gpu
GSC = 0.75                       # dLoss handed to the dlogits calls


def _model(case):
    from tests.test_gpu_attention import _make as make_attn
    from tests.test_gpu_decoder import _make_sized
    family, cell, _, E, H, V, L, _ = S.CASES[case]
    params = S.inputs(case)[0]
    if family == "attn":
        return make_attn(cell, {k: v.clone() for k, v in params.items()}, torch.float32).train()
    return _make_sized(cell, params, S.torch_dtype(case), E, H, V, L)


def _loss(case, m, feat, cap, lens, alpha_c, **kw):
    if S.CASES[case][0] == "attn":
        return m.loss(feat, cap, lens, alpha_c, **kw)
    return m.loss(feat, cap, lens, **kw)


def _run(case, m, **kw):
    """loss and every gradient of one loss() + backward on the case's inputs."""
    _, feat, cap, lens, alpha_c = S.inputs(case)
    for p in m.parameters():
        p.grad = None
    fd = feat.cuda().requires_grad_(True)
    loss = _loss(case, m, fd, cap.cuda(), lens, alpha_c, **kw)
    loss.backward()
    torch.cuda.synchronize()
    g = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    if S.CASES[case][0] != "attn":
        g["feat"] = fd.grad.detach().clone()
    return loss.item(), g


class _Rows:
    """One teacher-forced pass of the case up to the loss: what the C loss entry points take.  Fused route: the workspace of
    st_rnn_forward; launch chain: the logits rows in the dtype rnn.loss hands to st_cross_entropy."""

    def __init__(self, case, fused):
        from showtell_amd._lib import check, dtype_code, lib
        from showtell_amd.rnn import _cp, _stream, up8
        from showtell_amd.seq import plan_for
        self.case, self.m = case, _model(case)
        m = self.m
        _, feat, cap, lens, _ = S.inputs(case)
        self.V, self.n = m.vocab_size, sum(lens)
        self.target = R.pack_rows(cap, lens)
        capd = cap.cuda().contiguous()
        with torch.no_grad():
            out = m(feat.cuda(), capd, lens)
            self.fwd_logits = (out[0] if S.CASES[case][0] == "attn" else out).double().cpu()      # forward()'s fp32 logits
        self.fused = False
        if S.CASES[case][0] == "attn":
            with torch.no_grad():
                self.logits = m(feat.cuda(), capd, lens)[0].contiguous()
            self.targets = self.target.cuda()
            self.ldl, self.ldd, self.ldt = self.V, up8(self.V), torch.float32
            return
        dt = m.compute_dtype
        self.plan = plan_for(lens, torch.device("cuda", torch.cuda.current_device()))
        self.seq = self.plan.c_struct(capd)
        self.prm, self.keep = m._c_params()
        self.keep.append(capd)
        self.nbytes = lib().st_rnn_workspace_bytes(C.byref(self.prm), C.byref(self.seq))
        self.ws = torch.empty(self.nbytes, device="cuda", dtype=torch.uint8)
        self.targets = torch.empty(self.n, device="cuda", dtype=torch.long)
        self.ldl = self.ldd = lib().st_rnn_vocab_ld(self.V)
        self.ldt = dt
        self.fused = fused == "1" and bool(lib().st_rnn_fused_loss_supported(C.byref(self.prm)))
        assert self.fused == (fused == "1" and dt == torch.bfloat16)
        self.logits = None if self.fused else torch.empty(self.n, self.ldl, device="cuda", dtype=dt)
        check(lib().st_rnn_forward(C.byref(self.prm), C.byref(self.seq), _cp(m._feature(feat.cuda())), _cp(self.ws), self.nbytes,
                                   _cp(self.logits), dtype_code(dt), self.ldl, _cp(self.targets), 1, None, None, _stream()), "st_rnn_forward")
        if self.fused:
            self.sb = lib().st_rnn_fused_loss_bytes(C.byref(self.prm), C.byref(self.seq))
            self.tb = lib().st_rnn_fused_loss_ls_bytes(C.byref(self.prm), C.byref(self.seq))
            assert self.tb == self.n * ((self.V + S.TILE - 1) // S.TILE) * 4
        assert self.ldd == S.ldd_of(case)

    def reference_rows(self):
        """The float64 logits the route's loss kernels see: forward()'s fp32 logits on the fused route (no logits tensor
        exists there), the chain's own rows otherwise."""
        return self.fwd_logits if self.fused else self.logits[:, :self.V].double().cpu()

    @staticmethod
    def _terms(eps, w, nll=None, u=None):
        """st_loss_terms of one call: eps None -> smoothing = 0 (the kernels without the term), else
        smoothing = 1 at label_smoothing = eps (0.0 included: the label-smoothing kernels)."""
        from showtell_amd._lib import LossTerms
        t = LossTerms()
        t.row_weight, t.nll_out, t.smooth_out = (None if x is None else x.data_ptr() for x in (w, nll, u))
        t.smoothing, t.label_smoothing = (0, 0.0) if eps is None else (1, eps)
        return t

    def loss(self, eps=None, w=None, want_nll=True, want_u=False):
        """One loss call through the C entry points: eps None -> smoothing = 0, else smoothing = 1.
        Returns dict(loss, nll, u, lse)."""
        from showtell_amd._lib import check, dtype_code, lib
        from showtell_amd.rnn import _cp, _stream
        n = self.n
        loss = torch.zeros((), device="cuda")
        nll = torch.full((n,), -1.0, device="cuda") if want_nll else None
        u = torch.full((n,), -1.0, device="cuda") if want_u else None
        out = dict(loss=loss, nll=nll, u=u, lse=None)
        t = self._terms(eps, w, nll, u if eps is not None else None)
        if self.fused:
            self.scratch = torch.empty(self.sb // 4, device="cuda")
            if eps is not None:
                tsum = torch.full((self.tb // 4,), float("nan"), device="cuda")
                t.tile_sums, t.tile_sums_bytes = tsum.data_ptr(), self.tb
            check(lib().st_rnn_fused_loss(C.byref(self.prm), C.byref(self.seq), _cp(self.ws), self.nbytes, _cp(self.targets),
                                          _cp(self.scratch), self.sb, C.byref(t), _cp(loss), None, _stream()), "st_rnn_fused_loss")
            out["lse"] = self.scratch[:n]
        else:
            check(lib().st_cross_entropy(_cp(self.logits), dtype_code(self.ldt), _cp(self.targets), n, self.V, self.ldl, C.byref(t), _cp(loss),
                                         None, 0, self.ldd, 1.0, None, _stream()), "st_cross_entropy")
        torch.cuda.synchronize()
        return out

    def dlogits(self, eps=None, w=None):
        """(n, ldd) rows of the gradient call that follows the last loss() (the fused route reads its logsumexp); 7.0 where the
        call wrote nothing."""
        from showtell_amd._lib import check, dtype_code, lib
        from showtell_amd.rnn import _cp, _stream
        n = self.n
        gsc = torch.full((), GSC, device="cuda")
        d = torch.full((n, self.ldd), 7.0, device="cuda", dtype=self.ldt)
        t = self._terms(eps, w)
        if self.fused:
            check(lib().st_rnn_fused_dlogits(C.byref(self.prm), C.byref(self.seq), _cp(self.ws), self.nbytes, _cp(self.targets),
                                             _cp(self.scratch), _cp(gsc), C.byref(t), _cp(d), self.ldd, None, _stream()), "st_rnn_fused_dlogits")
        else:
            dtc = dtype_code(self.ldt)
            check(lib().st_cross_entropy(_cp(self.logits), dtc, _cp(self.targets), n, self.V, self.ldl, C.byref(t), None, _cp(d), dtc,
                                         self.ldd, 1.0, _cp(gsc), _stream()), "st_cross_entropy")
        torch.cuda.synchronize()
        return d


@pytest.mark.parametrize("case,fused", S.ROUTES)
def test_smooth_out_rows_match_logsumexp_minus_mean_in_float64(case, fused):
    """smooth_out[r] = logsumexp(x_r) - mean_{v < V} x_r[v] through the C entry point, against float64 on the route's logits.
    Bound: 4 x the fp32-against-float64 floor of that quantity, computed on the CPU from the oracle's rows (never from the
    kernel); nll in place of u, a mean over ldd, masked lanes counted or a dropped tile are 10 x and more outside
    (tests/test_label_smoothing_inputs.py).  nll_out stays the unsmoothed -log p(target); two runs of the fused route are bit-equal."""
    rows = _Rows(case, fused)
    eps = S.eps_of(case)
    x = rows.reference_rows()
    got = rows.loss(eps, None, want_nll=True, want_u=True)
    u, nll = got["u"].double().cpu(), got["nll"].double().cpu()
    bound = S.u_bound(case)
    diff = (u - S.u_of(x)).abs().max().item()
    dn = (nll - S.nll_of(x, rows.target)).abs().max().item()
    print(f"MEASURE smooth_out {case} fused={fused}: max|u - u64| {diff:.3e} (bound {bound:.3e}, floor {S.u_floor(case):.3e}); "
          f"max|nll - nll64| {dn:.3e}")
    assert torch.isfinite(u).all() and diff <= bound
    assert dn <= bound                            # logsumexp minus one fp32 logit: the same arithmetic, the same bound
    if rows.fused:
        again = rows.loss(eps, None, want_nll=True, want_u=True)
        assert torch.equal(again["u"], got["u"]) and torch.equal(again["nll"], got["nll"])


@pytest.mark.parametrize("case,fused", S.ROUTES)
def test_eps_zero_through_the_new_entry_points_is_the_weighted_call_bit_for_bit(case, fused):
    """The LS instantiations (smoothing = 1) with eps = 0, with and without row weights, against smoothing = 0:
    logsumexp, nll_out and dlogits bit for bit -- the extra sum disturbs nothing -- and the loss bit for bit where its fp32
    atomics cannot reorder (the fused reduction adds one term per 64-token block: at most two blocks), to 1e-6 relative
    otherwise (st_cross_entropy adds one term per row)."""
    rows = _Rows(case, fused)
    n = rows.n
    for w in (None, S.lin_weights(n).cuda()):
        old = rows.loss(None, w)
        d_old = rows.dlogits(None, w)
        new = rows.loss(0.0, w, want_u=True)
        d_new = rows.dlogits(0.0, w)
        assert torch.equal(new["nll"], old["nll"]) and (new["nll"] > 0).all()
        assert torch.isfinite(new["u"]).all() and (new["u"] > 0).all()
        if rows.fused:
            assert torch.equal(new["lse"], old["lse"])
        assert torch.equal(d_new, d_old) and (d_new[:, rows.V:] == 0).all() and d_new[:, :rows.V].float().abs().max().item() > 0
        lo, ln = old["loss"].item(), new["loss"].item()
        print(f"MEASURE eps=0 {case} fused={fused} weights={w is not None}: loss {ln!r} against {lo!r}")
        if rows.fused and (n + 63) // 64 <= 2:
            assert ln == lo
        else:
            scale = (old["nll"].double() * (w.double().abs() if w is not None else 1.0)).sum().item() / n
            assert abs(ln - lo) <= 1e-6 * scale


@pytest.mark.parametrize("case,fused", S.ROUTES)
def test_dlogits_rows_gain_exactly_the_smoothing_term(case, fused):
    """d0 from the existing entry point and d_eps from the new one, row weights from {0, +-0.5, +-1, 2}: every element obeys
    |d_eps - (d0 + eps * gw * (onehot - 1/V))| <= 2^-8 (bf16) / 2^-22 (fp32) * (|d0| + |expected|), gw = w_r * dLoss / N_tok, and
    the pad columns V .. ldd are exactly zero.  A dropped term is about 38 x outside at eps = 0.3."""
    rows = _Rows(case, fused)
    eps, n, V = S.eps_of(case), rows.n, rows.V
    w = S.lin_weights(n)
    wd = w.cuda()
    rows.loss(None, wd)
    d0 = rows.dlogits(None, wd).double().cpu()
    rows.loss(eps, wd)
    de = rows.dlogits(eps, wd).double().cpu()
    gw = w.double() * GSC / n
    exp = S.dlogits_expected(case, d0, gw, rows.target, eps)
    bound = S.dlogits_bound(case, d0, exp)
    err = (de - exp).abs()
    ratio = (err / bound.clamp(min=1e-300)).max().item()
    moved = ((de - d0).abs() / bound.clamp(min=1e-300))[w != 0][:, :V].min().item()
    print(f"MEASURE dlogits {case} fused={fused}: worst |d_eps - expected| / bound {ratio:.3f}; least |d_eps - d0| / bound {moved:.1f}")
    assert torch.isfinite(de).all() and (err <= bound).all()
    assert (de[:, V:] == 0).all() and (d0[:, V:] == 0).all() and (de[w == 0] == 0).all()
    assert moved >= 10                                       # every element of every weighted row carries the term


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("case,fused", S.ROUTES)
def test_smoothed_loss_and_gradients_match_the_float64_oracle(case, fused, weighted, monkeypatch):
    """rnn.loss(.., label_smoothing=eps), eps 0.3 (bf16) / 0.1 (fp32), without weights and with signed sequence and token
    weights: every parameter's gradient and the feature's within tol * (max|g_ref(w+)| + max|g_ref(w-)|), tol 4e-2 (bf16) / 1e-3
    (fp32); dropping the smoothing in the backward pass is 3 x to 100 x outside (tests/test_label_smoothing_inputs.py).  The
    loss: 2e-2 * mean|w| (bf16), 1e-4 * mean|w| (+ 3e-5 for the attention decoder's unweighted term) in fp32, the bounds of
    tests/test_gpu_weighted_loss.py."""
    monkeypatch.setenv("ST_FUSED_CE", fused)
    ref = S.reference(case, weighted)
    m = _model(case)
    eps = S.eps_of(case)
    kw = {}
    if weighted:
        sw, tw = S.weights(case)
        kw = dict(sequence_weight=sw.cuda(), token_weight=tw)
    loss, g = _run(case, m, label_smoothing=eps, **kw)
    dt = S.dtype_name(case)
    mean_w = S.packed_weights(case).abs().mean().item() if weighted else 1.0
    bound = 2e-2 * mean_w if dt == "bf16" else 1e-4 * mean_w + (3e-5 if S.CASES[case][0] == "attn" else 0.0)
    what = f"MEASURE smoothed {case} fused={fused} weighted={weighted}"
    print(f"{what}: loss {loss:.6f} oracle {ref['loss']:.6f} diff {abs(loss - ref['loss']):.3e} bound {bound:.3e}")
    assert set(g) == set(ref["g"])
    S.assert_grads_within_linear_bound(g, ref, S.GRAD_TOL[dt], what)
    assert abs(loss - ref["loss"]) <= bound


@pytest.mark.parametrize("case,fused", S.ROUTES)
def test_the_smoothed_scalar_is_the_recombination_of_its_own_rows(case, fused):
    """The loss of the call against ((1 - eps) * nll_out + eps * smooth_out) times the weights, summed in float64 and divided by
    N_tok, to 1e-6 relative (of the sum of the terms' magnitudes): the scalar itself cannot see smoothing on these flat logits,
    its rows can."""
    rows = _Rows(case, fused)
    eps, n = S.eps_of(case), rows.n
    for w in (None, S.packed_weights(case).float().cuda()):
        got = rows.loss(eps, w, want_u=True)
        per = (1.0 - eps) * got["nll"].double() + eps * got["u"].double()
        wd = w.double() if w is not None else torch.ones_like(per)
        want, scale = (wd * per).sum().item() / n, (wd.abs() * per.abs()).sum().item() / n
        print(f"MEASURE scalar {case} fused={fused} weights={w is not None}: loss {got['loss'].item():.7f} recombined {want:.7f} "
              f"relative {abs(got['loss'].item() - want) / scale:.2e}")
        assert abs(got["loss"].item() - want) <= 1e-6 * scale
        plain = rows.loss(None, w)
        assert plain["loss"].item() != got["loss"].item()                 # and it is not the unsmoothed scalar


def test_label_smoothing_zero_is_the_plain_call_on_the_fp32_chain(monkeypatch):
    """label_smoothing=0.0 through Python takes the path the call always took, without weights and with them: the three loss entry
    points are wrapped by functions that raise when their st_loss_terms asks for the label-smoothing kernels (smoothing = 1), and
    loss() + backward() still run.  Loss and gradients then equal the plain
    call's to 1e-6 relative, the bound tests/test_gpu_weighted_loss.py gives "the order of the fp32 atomics only".  Bit for bit
    cannot be asked of them: st_cross_entropy adds one float atomic per row to the loss and the embedding gradient one per token,
    so the plain call does not reproduce its own bits either (measured on an MI355X: 5.315089225769043 and 5.315090179443359 from
    two identical plain calls).  The values that no atomic touches -- logsumexp, nll_out, dlogits -- are compared bit for bit
    through the C entry points above."""
    from showtell_amd._lib import lib
    case = "gru_fp32"
    m = _model(case)
    sw, _ = S.weights(case)

    def guard(real, i):
        def call(*a):
            if a[i] is not None and a[i]._obj.smoothing:             # argument i: NULL or the st_loss_terms by reference
                raise AssertionError("label_smoothing=0.0 reached the label-smoothing kernels")
            return real(*a)
        return call
    for kw in ({}, dict(sequence_weight=sw.cuda())):
        loss0, g0 = _run(case, m, **kw)
        with monkeypatch.context() as mp:
            for name, i in (("st_rnn_fused_loss", 7), ("st_rnn_fused_dlogits", 7), ("st_cross_entropy", 6)):
                mp.setattr(lib(), name, guard(getattr(lib(), name), i))
            loss1, g1 = _run(case, m, label_smoothing=0.0, **kw)
            with pytest.raises(AssertionError, match="reached the label-smoothing kernels"):
                _run(case, m, label_smoothing=0.1, **kw)              # the patch is in the way of the smoothed path
        same = sum(torch.equal(g1[k], g0[k]) for k in g0)
        print(f"MEASURE eps=0 python weights={bool(kw)}: loss {loss1!r} against {loss0!r}; {same} of {len(g0)} gradients bit-equal")
        assert abs(loss1 - loss0) <= 1e-6 * abs(loss0)
        for k in g0:
            assert (g1[k] - g0[k]).abs().max().item() <= 1e-6 * g0[k].abs().max().item(), k


# ---- Trainer(.., label_smoothing=0.3): ResNet-18 at 64 x 64, B = 4, fp32 -----------------------------------------------------
TR = dict(E=64, H=64, V=120, L=2, B=4, seed=2, lr=0.1, momentum=0.9, eps=0.3, steps=2)
HEAD = ("linear_secondlast_layer.weight", "linear_secondlast_layer.bias", "last_layer.weight", "last_layer.bias")


def _torch_loop(enc, dec, data, eps):
    """The reference's loop in float64 torch: CrossEntropyLoss(label_smoothing=eps), SGD with momentum."""
    c = TR
    po = {k: v.double().clone() for k, v in enc.items()}
    for k in HEAD:
        po[k].requires_grad_(True)
    do = {k: v.double().clone().requires_grad_(True) for k, v in dec.items()}
    crit = torch.nn.CrossEntropyLoss(label_smoothing=eps)
    bufs, losses = {}, []
    for img, cap, lens in data:
        logits = R.rnn_forward(do, R.encoder_forward(po, img.double(), 18, train=True), cap, lens)
        loss = crit(logits, R.pack_rows(cap, lens))
        loss.backward()
        with torch.no_grad():
            for name, t in list(do.items()) + [(k, po[k]) for k in HEAD]:
                bufs[name] = R.sgd_momentum_step(t, t.grad, bufs.get(name), c["lr"], c["momentum"])
                t.grad = None
        losses.append(loss.item())
    return losses, {k: v.detach() for k, v in do.items()}


def test_trainer_with_label_smoothing_follows_a_float64_torch_loop():
    """Two SGD steps of Trainer(.., label_smoothing=0.3) on a small fp32 configuration against the same loop in float64 torch
    with CrossEntropyLoss(label_smoothing=0.3): each step's loss to 1e-3 (relative to max(1, loss)), and every decoder
    parameter's UPDATE (trained - initial) to 1e-3 of the oracle's largest update of that parameter (plus half an fp32 ulp of the
    stored weight per step).  The loss alone could not
    tell: the same loop without smoothing has losses within the bound, but its updates are 100 x and more outside (asserted)."""
    from showtell_amd import optim
    from showtell_amd.cnn import ResNet
    from showtell_amd.rnn import RNN
    from showtell_amd.train import Trainer
    c = TR
    enc = R.init_encoder_params(18, c["E"], seed=c["seed"])
    dec = R.init_decoder_params(c["E"], c["H"], c["V"], c["L"], "gru", seed=c["seed"])
    data = []
    for i in range(c["steps"]):
        cap, lens = R.synthetic_captions(c["B"], c["V"], seed=c["seed"] + i, mean=6, std=1.5, lo=4, hi=9)
        data.append((torch.randn(c["B"], 3, 64, 64, generator=torch.Generator().manual_seed(c["seed"] + i)), cap, lens))
    cnn = ResNet(18, c["E"]); cnn.load_state_dict(enc); cnn = cnn.cuda().train()
    rnn = RNN(c["E"], c["H"], c["V"], c["L"]); rnn.load_state_dict(dec); rnn = rnn.cuda().train()
    opt = optim.SGD(Trainer.trainable_params(cnn, rnn), lr=c["lr"], momentum=c["momentum"])
    tr = Trainer(cnn, rnn, opt, label_smoothing=c["eps"])
    got = [tr.step(img.cuda(), cap.cuda(), lens).item() for img, cap, lens in data]
    tr.flush()
    torch.cuda.synchronize()
    ref, trained = _torch_loop(enc, dec, data, c["eps"])
    _, unsmoothed = _torch_loop(enc, dec, data, 0.0)
    print(f"MEASURE trainer: losses {got} oracle {ref}")
    for a, b in zip(got, ref):
        assert abs(a - b) < 1e-3 * max(1.0, abs(b)), (got, ref)
    sd = rnn.state_dict()
    for k, t in trained.items():
        upd = t - dec[k].double()
        scale = upd.abs().max().item()
        err = (sd[k].double().cpu() - t).abs().max().item()
        away = (unsmoothed[k] - t).abs().max().item()
        print(f"MEASURE trainer {k}: update {scale:.3e} err {err:.3e} ({err / scale:.2e} of it); unsmoothed loop {away / scale:.2f} of it")
        assert err <= 1e-3 * scale + c["steps"] * 2.0 ** -24 * t.abs().max().item(), k      # + the fp32 rounding of the stored weight, once per step
        assert away >= 1e-1 * scale, k
