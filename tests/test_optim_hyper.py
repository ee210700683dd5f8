"""The host side of the optimizers' clipping / weight-decay keywords: what they accept, what a checkpoint's param_groups carry
and what load_state_dict restores or refuses.  On CPU parameters (the reference builds its optimizer before .cuda()), so
nothing here touches a device."""
import pytest
import torch


def _params():
    return [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]


def test_default_checkpoints_keep_their_keys_and_values():
    from showtell_amd import optim
    sgd, adam = optim.SGD(_params(), lr=0.1, momentum=0.9), optim.Adam(_params())
    assert sgd.state_dict()["param_groups"][0] == {"lr": 0.1, "momentum": 0.9, "dampening": 0, "weight_decay": 0, "nesterov": False, "params": [0, 1]}
    assert adam.state_dict()["param_groups"][0] == {"lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0, "amsgrad": False, "params": [0, 1]}
    for opt in (sgd, adam):
        assert opt._clip_args() == (False, 0.0, 0.0)               # the old entry points
        assert opt.last_grad_norm is None and opt.last_clip_coef is None and opt.skipped_steps is None   # no device buffers yet
        assert opt.param_groups[0]["weight_decay"] == 0.0 and opt.param_groups[0]["max_grad_norm"] is None
    assert adam.param_groups[0]["decoupled_weight_decay"] is False


def test_set_keywords_reach_param_groups_and_the_checkpoint():
    from showtell_amd import optim
    sgd = optim.SGD(_params(), lr=0.1, weight_decay=0.1, max_grad_norm=5, skip_nonfinite=True)
    g = sgd.state_dict()["param_groups"][0]
    assert (g["weight_decay"], g["max_grad_norm"], g["skip_nonfinite"]) == (0.1, 5.0, True)
    assert sgd._clip_args() == (True, 0.1, 5.0)
    adamw = optim.AdamW(_params())
    g = adamw.state_dict()["param_groups"][0]
    assert g["weight_decay"] == 1e-2 and g["decoupled_weight_decay"] is True and "max_grad_norm" not in g and "skip_nonfinite" not in g
    assert isinstance(adamw, optim.Adam) and adamw._clip_args() == (True, 1e-2, 0.0)
    assert "decoupled_weight_decay" not in optim.Adam(_params(), weight_decay=0.1).state_dict()["param_groups"][0]      # absent = L2
    # each keyword alone selects the extended step; param_groups is read at every step, like lr
    assert optim.Adam(_params(), skip_nonfinite=True)._clip_args() == (True, 0.0, 0.0)
    opt = optim.Adam(_params())
    opt.param_groups[0]["max_grad_norm"] = 2.5
    assert opt._clip_args() == (True, 0.0, 2.5) and opt.max_grad_norm == 2.5
    for bad in (dict(weight_decay=-0.1), dict(max_grad_norm=0.0), dict(max_grad_norm=-1.0), dict(weight_decay=float("nan"))):
        with pytest.raises(ValueError):
            optim.SGD(_params(), lr=0.1, **bad)
        with pytest.raises(ValueError):
            optim.Adam(_params(), **bad)


def test_load_restores_the_new_hyper_parameters_and_still_refuses_the_rest():
    from showtell_amd import optim
    src = optim.AdamW(_params(), lr=3e-4, weight_decay=0.1, max_grad_norm=5.0, skip_nonfinite=True)
    dst = optim.Adam(_params())
    dst.load_state_dict(src.state_dict())                           # stashed (CPU parameters); the hyper-parameters apply at once
    g = dst.param_groups[0]
    assert (g["lr"], g["weight_decay"], g["decoupled_weight_decay"], g["max_grad_norm"], dst.skip_nonfinite) == (3e-4, 0.1, True, 5.0, True)
    # a torch.optim checkpoint with weight decay, which used to be refused
    t = torch.optim.SGD(_params(), lr=0.1, momentum=0.9, weight_decay=0.01)
    sgd = optim.SGD(_params(), lr=1.0, max_grad_norm=3.0)
    sgd.load_state_dict(t.state_dict())
    assert sgd.param_groups[0]["weight_decay"] == 0.01 and sgd.momentum == 0.9 and sgd.max_grad_norm == 3.0     # a key the file lacks is kept
    t = torch.optim.AdamW(_params(), lr=0.1)
    adam = optim.Adam(_params())
    adam.load_state_dict(t.state_dict())
    assert adam.param_groups[0]["weight_decay"] == 1e-2 and adam.param_groups[0]["decoupled_weight_decay"] is True
    for cls, bad in ((optim.SGD, dict(dampening=0.1)), (optim.SGD, dict(nesterov=True)), (optim.Adam, dict(amsgrad=True)),
                     (optim.Adam, dict(weight_decay=-1.0))):
        opt = cls(_params(), lr=0.1)
        sd = opt.state_dict()
        sd["param_groups"][0].update(bad)
        with pytest.raises(ValueError):
            opt.load_state_dict(sd)


def test_trainer_has_a_grad_norm_property():
    from showtell_amd.train import Trainer
    assert isinstance(Trainer.grad_norm, property)
    for fn in (Trainer.step, Trainer.step_self_critical):
        assert "max_grad_norm" in fn.__doc__
