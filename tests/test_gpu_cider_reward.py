"""CIDEr rewards on the device (csrc/cider.hip, st_cider_reward; evaluation.cider_reward_device, Trainer.step_self_critical) against
the float64 oracle of tests/_cider_reward_cases.py, where the score, the cases and the oracle are stated.

Bounds.  None comes from the kernel.
  score64   1e-10 absolute against the oracle: both sides are float64, a score is at most 10 (every normalised val_n <= 1) and is a
            few hundred operations, a device log / exp and a contraction setting away from the oracle's; every seeded fault of
            tests/test_cider_reward_inputs.py moves a score by more than 0.2.
  reward    2^-20, one float32 ulp at 10, against the oracle's score rounded to float32.
  advantage 2^-18 against train.self_critical_advantage on the oracle's float32 rewards: two one-ulp moves and the final rounding.
  Trainer   identical ids; rewards within 2^-20; losses within 2^-18 x mean |nll| (every sequence weight moves by at most 2^-18 and
            the loss is sum w nll / N_tok; mean |nll| from the host path's token_logp) plus the fp32 floor that
            tests/test_gpu_weighted_loss.py allows its own self-critical step, 1e-4 x mean |w| over the packed tokens.
After the "#": what the kernel measured on the MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import restatement as R
from showtell_amd import evaluation as E
from tests import _cider_reward_cases as K
from tests import test_cider_reward_inputs as KI

pytestmark = pytest.mark.gpu

SCORE_TOL = KI.SCORE_TOL                # 1e-10
ULP = 2.0 ** -20
ADV_TOL = 2.0 ** -18
_CACHE = {}


def _device_run(name, baseline):
    """one launch of the case with the baseline: (score64 (B, S + 1), reward, advantage, greedy reward) on the host"""
    key = (name, baseline)
    if key not in _CACHE:
        c = K.case(name)
        fn = E.cider_reward_device(c["references"], c["table"], K.END)
        greedy = None if c["greedy"] is None else c["greedy"].cuda()
        reward, adv, gr = fn.advantage(c["ids"].cuda(), c["lengths"].cuda(), baseline, greedy)
        torch.cuda.synchronize()
        assert reward.is_cuda and reward.dtype == torch.float32 and reward.shape == c["lengths"].shape
        _CACHE[key] = (fn.last_score64.cpu().numpy(), reward.cpu(), None if adv is None else adv.cpu(), None if gr is None else gr.cpu())
    return _CACHE[key]


def _baselines(name):
    return ("greedy", "mean") if K.case(name)["greedy"] is not None else ("mean",)


# score64 against the oracle, max |d|: mixed 8.9e-16, single 0, limits 2.2e-16, corpus 4.4e-16, grid 8.9e-16; reward against the
# rounded oracle and advantage against the host rule: 0 in every case
@pytest.mark.parametrize("name", K.CASES)
def test_scores_match_the_float64_oracle(name):
    want = K.oracle_scores(name)
    score, reward, _, gr = _device_run(name, _baselines(name)[0])
    d = np.abs(score - want)
    print(f"MEASURE {name}: score64 against the oracle max |d| {d.max():.2e} (bound {SCORE_TOL:.0e}); scores {want.min():.3f} .. {want.max():.3f}")
    assert np.isfinite(score).all() and d.max() <= SCORE_TOL
    S = reward.shape[1]
    want32 = torch.from_numpy(want.astype(np.float32))
    dr = (reward.double() - want32[:, :S].double()).abs().max().item()
    print(f"MEASURE {name}: reward against the rounded oracle max |d| {dr:.2e} (one ulp {ULP:.2e})")
    assert dr <= ULP
    assert torch.equal(reward, torch.from_numpy(score[:, :S].astype(np.float32)))      # reward IS score64 rounded
    if gr is not None:
        assert torch.equal(gr, torch.from_numpy(score[:, S].astype(np.float32)))
    if name == "single":
        assert (score == 0.0).all() and (reward == 0).all()
    if name == "mixed":
        assert score[2, 0] == 0.0                            # first token <end>
        assert score[0, 1] == score[0, 3]                    # the same caption at two widths: bit-identical


@pytest.mark.parametrize("name", K.CASES)
def test_advantages_match_the_host_rule_for_both_baselines(name):
    want = K.oracle_scores(name)
    for baseline in _baselines(name):
        score, reward, adv, _ = _device_run(name, baseline)
        host = K.host_advantage(want, baseline)
        d = (adv.double() - host.double()).abs().max().item()
        print(f"MEASURE {name} {baseline}: advantage against self_critical_advantage of the oracle's rewards max |d| {d:.2e} (bound {ADV_TOL:.2e})")
        assert d <= ADV_TOL
        # ... and it IS that rule on the device's own float32 rewards, bit for bit
        own = np.concatenate([reward.numpy(), score[:, -1:].astype(np.float32)], 1)
        if baseline == "greedy":
            assert torch.equal(adv, K.host_advantage(own, "greedy"))
        else:
            assert (adv.double() - K.host_advantage(own, "mean").double()).abs().max().item() <= ULP    # the order of the sum may differ
        if name == "single":
            assert (adv == 0).all()
        else:
            assert (adv != 0).any()


def test_a_sample_identical_to_the_greedy_caption_has_advantage_exactly_zero():
    c = K.case("mixed")
    assert K.cut(c["ids"][0, 1].tolist(), int(c["lengths"][0, 1])) == K.cut(c["greedy"][0].tolist(), c["greedy"].shape[1])
    _, reward, adv, gr = _device_run("mixed", "greedy")
    assert reward[0, 1] > 0 and adv[0, 1].item() == 0.0 and reward[0, 1] == gr[0]
    assert (adv[0, [0, 2]] != 0).all()


def test_the_reward_fn_call_and_a_second_call_are_bit_identical():
    c = K.case("mixed")
    fn = E.cider_reward_device(c["references"], c["table"], K.END)
    ids, lengths, greedy = c["ids"].cuda(), c["lengths"].cuda(), c["greedy"].cuda()
    plain = fn(ids, lengths)
    assert plain.is_cuda and plain.dtype == torch.float32 and plain.shape == (6, 3)
    assert (fn.last_score64[:, 3] == 0).all()                # no greedy ids: the last column is not written
    assert fn.advantage(ids, lengths, None)[1:] == (None, None)
    first = fn.advantage(ids, lengths, "greedy", greedy)
    s1 = fn.last_score64.clone()
    second = fn.advantage(ids, lengths, "greedy", greedy)
    torch.cuda.synchronize()
    assert torch.equal(s1, fn.last_score64) and all(torch.equal(a, b) for a, b in zip(first, second))
    assert torch.equal(plain, first[0]) and torch.equal(plain.cpu(), _device_run("mixed", "greedy")[1])
    batch = E.cider_reward_device(c["references"], None, K.END)                       # no table: df over these images
    assert torch.equal(batch(ids, lengths), plain)


def test_python_refusals_on_the_device():
    c = K.case("mixed")
    fn = E.cider_reward_device(c["references"], c["table"], K.END)
    ids, lengths = c["ids"].cuda(), c["lengths"].cuda()
    with pytest.raises(ValueError, match="lengths"):
        fn(ids, lengths + 20)
    with pytest.raises(ValueError, match="num_samples >= 2"):
        fn.advantage(ids[:, :1].contiguous(), lengths[:, :1].contiguous(), "mean")
    with pytest.raises(ValueError, match="greedy_ids"):
        fn.advantage(ids, lengths, "greedy")
    from showtell_amd import ShowTellHipError
    with pytest.raises(ShowTellHipError):
        fn(c["ids"], c["lengths"])


@pytest.mark.parametrize("what", sorted(KI.C_REFUSALS))
def test_the_c_entry_point_refuses_with_outputs_untouched(what):
    from showtell_amd import _lib
    L = _lib.lib()
    buf = torch.zeros(4096, device="cuda", dtype=torch.int64)
    outs = [torch.full((64,), 7.0, device="cuda", dtype=dt) for dt in (torch.float64, torch.float32, torch.float32)]
    kw, word = KI.C_REFUSALS[what]
    rc = KI.c_call(L, C.c_void_p(buf.data_ptr()), out=tuple(C.c_void_p(o.data_ptr()) for o in outs), **kw)
    assert rc != 0 and word in L.st_last_error().decode(), what
    torch.cuda.synchronize()
    assert all((o == 7).all() for o in outs) and (buf == 0).all()


# ---- Trainer.step_self_critical: host reward against device reward from identical state ------------------------------------------
SC = dict(E=64, H=64, V=50, L=2, B=4, S=3, seed=3)


class _Recorder:
    """a reward_fn that returns zeros and keeps what it was given (the probe step that the references are cut from)"""

    def __init__(self):
        self.calls = []

    def __call__(self, ids, lengths):
        self.calls.append((ids.clone(), lengths.clone()))
        return torch.zeros(tuple(lengths.shape))


class _HostReward(_Recorder):
    def __init__(self, references):
        super().__init__()
        self.fn, self.rewards = E.cider_reward(references, K.END), []

    def __call__(self, ids, lengths):
        self.calls.append((ids.clone(), lengths.clone()))
        self.rewards.append(self.fn(ids, lengths))
        return self.rewards[-1]


class _DeviceReward:
    def __init__(self, references):
        self.fn, self.seen = E.cider_reward_device(references, None, K.END), []

    def __call__(self, ids, lengths):
        return self.fn(ids, lengths)

    def advantage(self, ids, lengths, baseline, greedy_ids=None, **kw):
        out = self.fn.advantage(ids, lengths, baseline, greedy_ids, **kw)
        self.seen.append((ids, lengths, greedy_ids) + out)
        return out


def _plain_trainer():
    from showtell_amd import optim
    from showtell_amd.cnn import ResNet
    from showtell_amd.rnn import RNN
    from showtell_amd.train import Trainer
    c = SC
    enc = R.init_encoder_params(18, c["E"], seed=c["seed"])
    dec = R.init_decoder_params(c["E"], c["H"], c["V"], c["L"], "gru", seed=c["seed"])
    dec["linear.bias"][K.END] += 2.0                         # <end> likely enough that the samples end at different steps
    cnn = ResNet(18, c["E"]); cnn.load_state_dict(enc); cnn = cnn.cuda().train()
    rnn = RNN(c["E"], c["H"], c["V"], c["L"]); rnn.load_state_dict(dec); rnn = rnn.cuda().train()
    img = torch.randn(c["B"], 3, 64, 64, generator=torch.Generator().manual_seed(c["seed"])).cuda()
    tr = Trainer(cnn, rnn, optim.SGD(Trainer.trainable_params(cnn, rnn), lr=0.1, momentum=0.0))
    return tr, img, lambda: cnn(img)


ATTN = dict(F=32, A=32, P=9)


def _attention_trainer():
    """The attention decoder reads a frozen feature map, so its Trainer has no trainable head: `_features` hands the map over."""
    from showtell_amd import optim
    from showtell_amd.train import Trainer
    from tests.test_gpu_attention import _make
    c = SC

    class FixedFeatures(Trainer):
        def _features(self, image, upcoming):
            self._apply_pending()
            self.opt.zero_grad()
            return image

    dec = R.init_decoder_params(c["E"], c["H"], c["V"], c["L"], "gru", seed=c["seed"], attn=dict(F=ATTN["F"], A=ATTN["A"]))
    dec["linear.bias"][K.END] += 2.0
    rnn = _make("gru", dec, torch.float32).train()
    feat = torch.randn(c["B"], ATTN["F"], ATTN["P"], generator=torch.Generator().manual_seed(c["seed"])).abs().cuda()
    tr = FixedFeatures(None, rnn, optim.SGD(list(rnn.parameters()), lr=0.1, momentum=0.0))
    return tr, feat, lambda: feat


def _references_from(samples, greedy):
    """per image: its first sample, a sample of the next image, and a splice of two of its own; never empty"""
    B, S, T = samples.shape
    words = lambda row: K.cut(row.tolist(), T) or [5, 6, 7]
    refs = []
    for b in range(B):
        a, n, z = words(samples[b, 0]), words(samples[(b + 1) % B, 1]), words(samples[b, 2])
        refs.append([a, n, (a[:3] + z[1:])[:20]] + ([words(greedy[b])] if greedy is not None and b % 2 else []))
    return refs


# ids identical in all three; rewards max |d| 0; loss |d| over three runs (the loss kernels' own run-to-run spread): plain greedy
# 0 to 1.4e-06 of 2.1e-04, plain mean 0 to 2.4e-06 of 2.3e-04, attention mean 0 to 1.4e-06 of 2.4e-04
@pytest.mark.parametrize("kind,baseline", [("plain", "greedy"), ("plain", "mean"), ("attn", "mean")])
def test_trainer_steps_with_the_host_and_the_device_reward_agree(kind, baseline):
    """Two trainers from identical state and uniforms.  (The attention decoder's greedy decode takes a vocabulary object, which
    step_self_critical does not pass: its comparison runs the 'mean' baseline.)"""
    from showtell_amd.rnn import CAP_MAX
    from showtell_amd.train import sample_caption_batch, self_critical_advantage
    make = _plain_trainer if kind == "plain" else _attention_trainer
    B, S = SC["B"], SC["S"]
    u = torch.rand(B, S, CAP_MAX, generator=torch.Generator().manual_seed(11)).cuda()
    probe, x, features = make()
    rec = _Recorder()
    probe.step_self_critical(x, rec, num_samples=S, baseline=baseline, uniforms=u)
    samples = rec.calls[-1][0]
    refs = _references_from(samples, rec.calls[0][0][:, 0] if baseline == "greedy" else None)

    host_tr, xh, _ = make()
    host = _HostReward(refs)
    loss_h, mean_h = host_tr.step_self_critical(xh, host, num_samples=S, baseline=baseline, uniforms=u)
    dev_tr, xd, _ = make()
    dev = _DeviceReward(refs)
    loss_d, mean_d = dev_tr.step_self_critical(xd, dev, num_samples=S, baseline=baseline, uniforms=u)
    torch.cuda.synchronize()

    ids_h, len_h = host.calls[-1]
    ids_d, len_d, gids_d, reward_d, adv_d, greedy_d = dev.seen[0]
    assert len(dev.seen) == 1 and ids_d.is_cuda and reward_d.is_cuda and adv_d.is_cuda and mean_d.is_cuda and mean_d.dim() == 0
    assert torch.equal(ids_d.cpu(), ids_h) and torch.equal(len_d.cpu(), len_h) and torch.equal(ids_h, samples)
    reward_h = host.rewards[-1]
    if baseline == "greedy":
        assert torch.equal(gids_d.cpu(), host.calls[0][0][:, 0])
        assert (greedy_d.cpu() - host.rewards[0][:, 0]).abs().max().item() <= ULP
    dr = (reward_d.cpu().double() - reward_h.double()).abs().max().item()
    adv_h = self_critical_advantage(reward_h, baseline, host.rewards[0] if baseline == "greedy" else None)
    assert (reward_h > 0.5).sum() >= B and (adv_h != 0).sum() >= B * S // 2            # rewards and weights that matter
    assert len(set(len_h.reshape(-1).tolist())) >= 3                                    # ragged rows
    # the bound: every sequence weight moves by at most 2^-18, and loss = sum_tokens w * nll / N_tok; plus the fp32 floor
    order, cap, lens = sample_caption_batch(ids_h, len_h)
    with torch.no_grad():
        nll = -probe.rnn.token_logp(features()[(order // S).cuda()], cap.cuda(), lens).double().cpu()
    ntok = float(sum(lens))
    mean_nll = nll.abs().sum().item() / ntok
    mean_w = sum(abs(float(a)) * l for a, l in zip(adv_h.reshape(-1)[order].tolist(), lens)) / ntok
    bound = ADV_TOL * mean_nll + 1e-4 * mean_w
    dl = abs(loss_d.item() - loss_h.item())
    print(f"MEASURE trainer {kind} {baseline}: rewards max |d| {dr:.2e} (bound {ULP:.2e}); loss host {loss_h.item():.6f} device {loss_d.item():.6f} "
          f"|d| {dl:.2e} (bound {bound:.2e}: mean |nll| {mean_nll:.3f}, mean |w| {mean_w:.3f}); lens {lens}")
    assert dr <= ULP
    assert abs(mean_d.item() - float(mean_h)) <= ULP
    assert loss_h.item() != 0.0 and dl <= bound
    for t in (probe, host_tr, dev_tr):
        t.flush()
