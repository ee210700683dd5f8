"""Scheduled sampling without a GPU: the numpy replica of the mix rule on the cases' uniforms, the schedules' known values, the
host-side argument errors, and the proof from the float64 oracles alone that the inputs and bounds of
tests/test_gpu_scheduled_sampling.py catch the faults they are meant to catch (tests/_scheduled_sampling_cases.py).

Power.  Each seeded fault is expressed in the oracle and handed to the very checks the GPU tests make:
  roll-in (test 3: rollin_violations)   the comparison flipped; replacement shifted by one slot; a slot past the length replaced;
                                        the draw taken from the logits one step off
  loss (test 4: the linear-form gradient bound and the loss bound)
                                        the embedding gradient scattered by the caption; the targets taken from input_ids
and every one must be reported.  The cases' rate and seeds give every case a row with replaced and unreplaced valid slots."""
import numpy as np
import pytest
import torch

from tests import _scheduled_sampling_cases as K


# ---- the mix rule ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(K.CASES))
def test_mix_rule_on_the_cases_uniforms(case):
    _, _, cap, lens, _ = K.inputs(case)
    kind = K.family(case)
    coin = K.uniforms(case)[0].numpy()
    B, T = cap.shape
    assert lens[-1] == 1 and lens[-2] == 2 and len(set(lens)) > 2            # unequal lengths, a length-1 and a length-2 row
    valid = K.valid_slots(kind, lens, T)
    for b in range(B):                                                       # the rule, slot by slot, in plain Python
        for j in range(T):
            fed = j + 1 if kind == "rnn" else j                              # the step slot j feeds
            want = fed < lens[b] and (kind == "rnn" or j >= 1)
            assert valid[b, j] == want
    assert not valid[-1].any()                                               # a length-1 row has nothing to replace
    assert valid[-2].sum() == 1                                              # a length-2 row exactly one slot (slot 0 / slot 1)
    assert valid.sum() == sum(lens) - B                                      # every fed step but the first of each row
    rep = K.mix_rule(kind, lens, coin, K.P)
    assert np.array_equal(rep, valid & (coin < np.float32(K.P)))
    assert not K.mix_rule(kind, lens, coin, 0.0).any()                       # strict: p = 0 replaces nothing
    assert np.array_equal(K.mix_rule(kind, lens, coin, 1.0), valid)          # p = 1 every valid slot (uniforms are < 1)
    at = np.float32(coin[0, 1])
    assert not K.mix_rule(kind, lens, coin, at)[0, 1]                        # coin == p exactly: not replaced
    assert K.mix_rule(kind, lens, coin, np.nextafter(at, np.float32(2)))[0, 1] == valid[0, 1]
    both = [(rep[b] & valid[b]).any() and (~rep[b] & valid[b]).any() for b in range(B)]
    assert any(both), "no row with replaced and unreplaced valid slots"
    drawn = np.full(cap.shape, 7)
    mixed = K.mix_tokens(cap.numpy(), drawn, rep)
    assert (mixed[rep] == 7).all() and np.array_equal(mixed[~rep], cap.numpy()[~rep])


# ---- the schedules ---------------------------------------------------------------------------------------------------------

def test_the_schedules_known_values():
    from showtell_amd.train import inverse_sigmoid_ss_schedule, linear_ss_schedule
    f = linear_ss_schedule(0.0, 0.25, 100)
    assert f(0) == 0.0 and f(50) == 0.125 and f(100) == 0.25 and f(10 ** 9) == 0.25
    g = linear_ss_schedule(1.0, 0.5, 4)
    assert [g(i) for i in range(6)] == [1.0, 0.875, 0.75, 0.625, 0.5, 0.5]
    h = inverse_sigmoid_ss_schedule(10.0)
    assert h(0) == pytest.approx(1.0 / 11.0, abs=1e-15)                      # 1 - k / (k + 1)
    assert h(10) == pytest.approx(1.0 - 10.0 / (10.0 + np.e), abs=1e-15)
    assert all(h(i) < h(i + 1) for i in range(0, 200, 7)) and h(10 ** 7) == 1.0 and 0.0 <= h(0) <= 1.0
    for bad in (lambda: linear_ss_schedule(-0.1, 0.5, 10), lambda: linear_ss_schedule(0.0, 1.5, 10), lambda: linear_ss_schedule(0.0, 0.5, 0),
                lambda: inverse_sigmoid_ss_schedule(0.5)):
        with pytest.raises(ValueError):
            bad()


# ---- host-side argument errors ---------------------------------------------------------------------------------------------

def _cpu_decoders():
    from showtell_amd.rnn import RNN
    from showtell_amd.rnn_attn import RNN_Attn
    return [(RNN(8, 8, 20, 1), torch.zeros(3, 8)), (RNN_Attn(8, 8, 8, 8, 20, 1), torch.zeros(3, 8, 49))]


@pytest.mark.parametrize("which", [0, 1])
def test_argument_errors_are_raised_before_the_device_is_touched(which):
    """On CPU tensors: a ValueError, not the 'needs a HIP device' error that anything later would raise."""
    m, feat = _cpu_decoders()[which]
    cap = torch.tensor([[1, 5, 6, 2], [1, 7, 2, 0], [1, 2, 0, 0]])
    lens = [4, 3, 2]
    ok = torch.zeros(2, 3, 4)
    for bad in (dict(p=-0.1), dict(p=1.5), dict(p=float("nan")), dict(p="x"), dict(p=0.5, temperature=0.0), dict(p=0.5, top_k=33),
                dict(p=0.5, top_k=21), dict(p=0.5, top_k=-1), dict(p=0.5, uniforms=torch.zeros(3, 4)), dict(p=0.5, uniforms=torch.zeros(2, 3, 5)),
                dict(p=0.5, uniforms=ok.double()), dict(p=0.5, uniforms=ok.to("meta"))):
        with pytest.raises(ValueError):
            m.scheduled_inputs(feat, cap, lens, **bad)
    with pytest.raises(ValueError):
        m.scheduled_inputs(feat, cap.int(), lens, 0.5)
    with pytest.raises(ValueError):
        m.scheduled_inputs(feat, cap, [4, 3], 0.5)
    with pytest.raises(ValueError):
        m.scheduled_inputs(feat[:2], cap, lens, 0.5)
    for call in (m.loss, m.forward, m.token_logp):
        for ids in (cap[:, :3], cap.int(), cap.clone().fill_(20), cap.clone().fill_(-1), cap.to("meta"), [1, 2]):
            with pytest.raises(ValueError):
                call(feat, cap, lens, input_ids=ids)
    for bad in (dict(scheduled_sampling=1.5), dict(scheduled_sampling=-1), dict(scheduled_sampling=0.5, input_ids=cap),
                dict(scheduled_sampling=0.5, ss_top_k=40), dict(scheduled_sampling=0.5, ss_uniforms=torch.zeros(3, 4))):
        with pytest.raises(ValueError):
            m.loss(feat, cap, lens, **bad)


def test_trainer_refuses_a_bad_rate():
    from showtell_amd.train import Trainer
    with pytest.raises(ValueError):
        Trainer(None, None, None, scheduled_sampling=1.5)


# ---- the cases' power ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(K.CASES))
def test_the_roll_in_checks_pass_the_oracle_and_catch_every_fault(case):
    ids, rep, lp = K.oracle_roll_in(case)
    assert K.rollin_violations(case, ids, rep) == []                         # the oracle obeys its own rule exactly
    lo, hi = K.interval_excess(lp, ids, K.uniforms(case)[1])
    assert (lo[rep] <= 0).all() and (hi[rep] < 0).all()
    assert int(rep.sum()) >= 4
    for fault in K.FAULTS:
        fids, frep, _ = K.oracle_roll_in(case, fault)
        found = K.rollin_violations(case, fids, frep)
        print(f"MEASURE {case} fault {fault}: {found}")
        assert found, f"{case}: the fault '{fault}' passes the checks of the GPU test"


LOSS_RUNS = [(c, "plain") for c in K.CASES] + [(c, "w_ls") for c in K.CASES] + [("gru777", "dropout")]


@pytest.mark.parametrize("case,variant", LOSS_RUNS)
def test_the_loss_bounds_catch_both_faults(case, variant):
    ref = K.loss_reference(case, variant)
    tol = K.GRAD_TOL[K.dtype_name(case)]
    assert K.grad_violations(ref["g"], ref, tol) == []
    assert len(K.target_only_tokens(case)) >= 2 and {1, 2} <= set(K.target_only_tokens(case))
    X, cap = K.random_ids(case), K.inputs(case)[2]
    assert (X != cap).all()
    # the embedding rows of tokens that only the targets hold: exactly zero in the oracle too
    assert (ref["g"]["embeddings.weight"][K.target_only_tokens(case)] == 0).all()
    for fault in K.LOSS_FAULTS:
        bad = K.loss_reference(case, variant, fault)
        out = K.grad_violations(bad["g"], ref, tol)
        dl = abs(bad["loss"] - ref["loss"])
        print(f"MEASURE {case} {variant} fault {fault}: gradients outside {out}; |d loss| {dl:.3e} (bound {K.loss_bound(case, ref):.3e})")
        assert out or dl > K.loss_bound(case, ref), f"{case} {variant}: the fault '{fault}' stays inside every bound"
        if fault == "emb_grad_by_caption":
            assert "embeddings.weight" in out
            assert (bad["g"]["embeddings.weight"][K.target_only_tokens(case)] != 0).any()      # and the exact-zero check sees it
