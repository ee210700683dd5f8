"""The host side of the weighted loss, token_logp and the self-critical step, and the proof from the float64 oracle alone that
the weights tests/test_gpu_weighted_loss.py uses give its gradient bound power.  Nothing here needs a GPU."""
import numpy as np
import pytest
import torch

from oracle import restatement as R
from tests import _weighted_loss_cases as W


def _cpu_decoders():
    from showtell_amd.rnn import RNN
    from showtell_amd.rnn_attn import RNN_Attn
    from showtell_amd.rnn_lstm import RNN as RNN_LSTM
    return [(RNN(8, 8, 20, 1), torch.zeros(3, 8)), (RNN_LSTM(8, 8, 20, 1), torch.zeros(3, 8)),
            (RNN_Attn(8, 8, 8, 8, 20, 1), torch.zeros(3, 8, 49))]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_argument_errors_are_raised_before_the_device_is_touched(which):
    """On CPU tensors: a ValueError, not the 'needs a HIP device' error that anything later would raise."""
    from showtell_amd import ShowTellHipError
    m, feat = _cpu_decoders()[which]
    cap, lens = torch.tensor([[1, 5, 6, 2], [1, 7, 2, 0], [1, 2, 0, 0]]), [4, 3, 2]
    for bad in (dict(sequence_weight=torch.zeros(2)), dict(sequence_weight=torch.zeros(3, 1)), dict(sequence_weight=torch.zeros(3, dtype=torch.long)),
                dict(sequence_weight=[0.0, 1.0, 2.0]), dict(token_weight=torch.zeros(3, 3)), dict(token_weight=torch.zeros(3)),
                dict(token_weight=torch.zeros(4, 3)), dict(token_weight=torch.zeros(3, 4, dtype=torch.int32)),
                dict(sequence_weight=torch.zeros(3), token_weight=torch.zeros(3, 5))):
        with pytest.raises(ValueError):
            m.loss(feat, cap, lens, **bad)
    for bad_cap, bad_lens in ((cap.int(), lens), (cap[0], lens), (cap, [4, 3]), (cap, [5, 3, 2])):
        with pytest.raises(ValueError):
            m.token_logp(feat, bad_cap, bad_lens)
        with pytest.raises(ValueError):
            m.loss(feat, bad_cap, bad_lens, sequence_weight=torch.zeros(3))
    # well-formed arguments get as far as the device check: there is no CPU route
    with pytest.raises(ShowTellHipError):
        m.loss(feat, cap, lens, sequence_weight=torch.ones(3, dtype=torch.float64), token_weight=torch.ones(3, 4))
    with pytest.raises(ShowTellHipError):
        m.token_logp(feat, cap, lens)


def test_weights_are_gathered_to_packed_rows_like_pack_rows():
    """pack_row_weights / unpack_rows (the plan's rows_b / rows_t) against the oracle's pack_rows, on a ragged batch with a
    caption tensor wider than the longest caption."""
    from showtell_amd.rnn import pack_row_weights, unpack_rows
    from showtell_amd.seq import plan_for
    lens = [7, 5, 5, 2, 1]
    plan = plan_for(lens, torch.device("cpu"))
    g = torch.Generator().manual_seed(4)
    sw, tw = torch.randn(5, generator=g, dtype=torch.float64), torch.randn(5, 9, generator=g)
    assert pack_row_weights(plan, None, None, "cpu") is None
    ref_s = R.pack_rows(sw.float()[:, None].expand(5, 9), lens)
    ref_t = R.pack_rows(tw, lens)
    for got, ref in ((pack_row_weights(plan, sw, None, "cpu"), ref_s), (pack_row_weights(plan, None, tw, "cpu"), ref_t),
                     (pack_row_weights(plan, sw, tw, "cpu"), ref_s * ref_t)):
        assert got.dtype == torch.float32 and got.shape == (plan.ntok,) and got.is_contiguous() and not got.requires_grad
        assert torch.equal(got, ref)
    # no gradient flows into the weights
    assert not pack_row_weights(plan, sw.clone().requires_grad_(True), None, "cpu").requires_grad
    # and back: rows -> (B, T), zero past each length
    rows = torch.arange(1, plan.ntok + 1, dtype=torch.float32)
    back = unpack_rows(plan, rows, 9, "cpu")
    assert back.shape == (5, 9) and torch.equal(R.pack_rows(back, lens), rows)
    for b, l in enumerate(lens):
        assert (back[b, :l] != 0).all() and (back[b, l:] == 0).all()


def test_cider_reward_on_ids_equals_cider_score_on_the_same_captions_as_strings():
    from showtell_amd.evaluation import cider_reward, cider_score
    rng = np.random.RandomState(3)
    B, S, T, V = 5, 3, 9, 12
    refs = [[[1] + rng.randint(4, V, size=rng.randint(3, 7)).tolist() + [2] for _ in range(rng.randint(1, 4))] for _ in range(B)]
    ids = np.zeros((B, S, T), dtype=np.int64)
    lengths = np.zeros((B, S), dtype=np.int64)
    words = [[None] * S for _ in range(B)]
    for b in range(B):
        for s in range(S):
            body = rng.randint(4, V, size=rng.randint(1, 6)).tolist()
            if s == 0:
                body = refs[b][0][1:-1]                    # one sample per image repeats a reference
            ended = (b + s) % 3 != 0                        # some rows never draw <end>: their length is what sample reports
            row = [1] + body + ([2] if ended else [])
            ids[b, s, :len(row)] = row
            lengths[b, s] = len(row)
            words[b][s] = [1] + body
    fn = cider_reward(refs)
    got = fn(torch.from_numpy(ids), torch.from_numpy(lengths))
    assert isinstance(got, torch.Tensor) and got.shape == (B, S) and got.dtype == torch.float32
    gts = {b: [" ".join(str(t) for t in r[:-1]) for r in refs[b]] for b in range(B)}
    for s in range(S):
        res = {b: [" ".join(str(t) for t in words[b][s])] for b in range(B)}
        np.testing.assert_allclose(got[:, s].numpy(), cider_score(gts, res)[1], rtol=1e-6, atol=1e-7)
    assert got[:, 0].min() > got[:, 1:].max()               # the repeated reference scores highest
    with pytest.raises(ValueError):
        fn(torch.from_numpy(ids[:2]), torch.from_numpy(lengths[:2]))


def test_self_critical_sort_and_advantage_bookkeeping():
    """sample_caption_batch on a hand-made ragged batch: stable descending sort, the image and the value of every sorted row."""
    from showtell_amd.train import sample_caption_batch, self_critical_advantage
    lengths = torch.tensor([[3, 5], [5, 2], [4, 5]])
    B, S, T = 3, 2, 6
    ids = torch.zeros(B, S, T, dtype=torch.long)
    for b in range(B):
        for s in range(S):
            ids[b, s, :lengths[b, s]] = 100 * b + 10 * s + torch.arange(1, lengths[b, s] + 1)
    order, cap, lens = sample_caption_batch(ids, lengths)
    assert order.tolist() == [1, 2, 5, 4, 0, 3]             # the three rows of length 5 keep their order
    assert lens == [5, 5, 5, 4, 3, 2]
    assert (order // S).tolist() == [0, 1, 2, 2, 0, 1]      # the image whose feature every sorted row gets
    for k, o in enumerate(order.tolist()):
        assert torch.equal(cap[k], ids[o // S, o % S])
    reward = torch.tensor([[1.0, 4.0], [2.0, 2.0], [0.0, 6.0]])
    adv = self_critical_advantage(reward, "greedy", torch.tensor([[1.0], [3.0], [2.0]]))
    assert torch.equal(adv, torch.tensor([[0.0, 3.0], [-1.0, -1.0], [-2.0, 4.0]]))
    assert adv.reshape(-1)[order].tolist() == [3.0, -1.0, 4.0, -2.0, 0.0, -1.0]
    # un-sort: the inverse permutation puts a per-row value back at (b, s)
    inv = torch.empty_like(order); inv[order] = torch.arange(B * S)
    assert torch.equal(adv.reshape(-1)[order][inv].view(B, S), adv)
    # 'mean': the mean of the image's OTHER samples
    r3 = torch.tensor([[1.0, 2.0, 6.0], [0.0, 0.0, 3.0]])
    assert torch.allclose(self_critical_advantage(r3, "mean"), torch.tensor([[-3.0, -1.5, 4.5], [-1.5, -1.5, 3.0]]))
    assert torch.equal(self_critical_advantage(torch.full((2, 3), 0.7), "mean"), torch.zeros(2, 3))
    assert torch.equal(self_critical_advantage(torch.full((2, 3), 0.7), "greedy", torch.full((2, 1), 0.7)), torch.zeros(2, 3))
    for bad in (lambda: self_critical_advantage(r3, "median"), lambda: self_critical_advantage(r3[:, :1], "mean"),
                lambda: self_critical_advantage(r3, "greedy", torch.zeros(3))):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("case", sorted(W.CASES))
def test_the_weights_have_both_signs_and_the_gradient_bound_has_power(case):
    """The weights of the GPU test's oracle comparison: both signs per sequence, per token and on the packed rows; and for every
    parameter (and the feature) max|g_ref(w)| is at least 5 % of max|g_ref(w+)| + max|g_ref(w-)|, the scale its bound is
    relative to -- a kernel that ignored the weights, or applied the wrong row's, could not hide inside it."""
    sw, tw = W.weights(case)
    _, _, cap, lens, _ = W.inputs(case)
    w = W.packed_weights(case)
    assert sw.shape == (cap.shape[0],) and tw.shape == tuple(cap.shape) and w.shape == (sum(lens),)
    for t in (sw, tw, w):
        assert (t > 0).any() and (t < 0).any() and t.abs().max() <= 1
    ref = W.reference(case)
    for k in ref["g"]:
        if k in W.ZERO_GRADS:
            assert ref["g"][k].abs().max().item() < 1e-12, k         # analytically zero: float64 noise
            continue
        own, scale = ref["g"][k].abs().max().item(), W.grad_scale(ref, k)
        print(f"MEASURE {case} {k}: max|g(w)| {own:.3e}  scale {scale:.3e}  ratio {own / scale:.3f}")
        assert own >= 0.05 * scale, (k, own, scale)
    # ... and the unweighted gradient is not inside the bound either: ignoring the weights would be caught
    params, feat, cap, lens, alpha_c = W.inputs(case)
    plain = W.oracle_grads(case, params, feat, cap, lens, torch.ones_like(w), alpha_c, feat_grad="feat" in ref["g"])["g"]
    tol = W.GRAD_TOL[W.CASES[case][2]]
    caught = [k for k in ref["g"] if k not in W.ZERO_GRADS and (plain[k] - ref["g"][k]).abs().max().item() > tol * W.grad_scale(ref, k)]
    assert len(caught) == len([k for k in ref["g"] if k not in W.ZERO_GRADS]), set(ref["g"]) - set(caught)
