"""The inputs and the torch replica that tests/test_grad_clip_inputs.py and tests/test_gpu_grad_clip.py share.

Five parameter tensors of 1, 3, 35, 2112 and 1025 elements (every 4-element padding case of the flat buffer, a tail shorter
than one vector; 3184 padded elements) and six steps of synthetic gradients: every element is +-U[0.5, 2) times the step's
scale, so that g / sqrt(v) stays well conditioned and Adam needs no noise-floor allowance.  The scales 1, 1, 30, 0.01, 1, 1
give global norms of about 74, inf, 2236, 0.74, 74, 74: with MAX_NORM = 5 the clip is active on four steps and inactive on
one, and the second step, which has one +inf element, is the one to skip -- where Adam's bias correction is most sensitive
to a wrong step count.  A second, long set (LONG_SHAPES, long_params(), long_grads(); replica(long=True)) takes the step kernels past
their grid cap.

The replica is plain torch on CPU copies: global norm; skip the iteration if it is not finite; else
p.grad.mul_(min(1, max / (norm + 1e-6))); then torch.optim.SGD / Adam / AdamW .step().  In float64 it is the reference, in
float32 it measures the reference's own error, and with one of FAULTS seeded it shows that the bound can tell.  Everything is
computed once per process (lru_cache) and handed out as is: callers do not modify it."""
import functools

import torch

SHAPES = [(1,), (3,), (5, 7), (64, 33), (1025,)]
SCALES = [1.0, 1.0, 30.0, 0.01, 1.0, 1.0]
NAN_STEP, INF_AT = 1, (2, 17)        # step index; (tensor index, flat element) that is +inf there
MAX_NORM, WEIGHT_DECAY = 5.0, 0.1
KINDS = ("SGD", "Adam", "AdamW")
HYPER = {"SGD": dict(lr=0.05, momentum=0.9), "Adam": dict(lr=1e-3), "AdamW": dict(lr=1e-3)}
# max|p_got - p_ref| / max|p_ref| after the six steps.  From the reference: the float32 replica differs from the float64 one by
# 1.3e-7 (SGD), 1.4e-7 (Adam), 2.1e-7 (AdamW); ten times the largest leaves room for fused multiply-add and another summation order.
BOUND = 2e-6
# fault: the kinds it applies to
FAULTS = {
    "no_clip": KINDS,                          # the coefficient is never applied
    "per_tensor_norm": KINDS,                  # every tensor clipped to MAX_NORM by its own norm
    "no_decay": KINDS,                         # weight decay dropped
    "decay_swapped": ("Adam", "AdamW"),        # L2 where decoupled was asked for, and the reverse
    "coef_after_decay": ("SGD", "Adam"),       # coef * (g + wd * p) instead of coef * g + wd * p
    "skip_counts": ("Adam", "AdamW"),          # the skipped step still advances the bias-correction count
}


@functools.lru_cache(maxsize=None)
def params():
    """The starting parameters, fp32 CPU, N(0, 1)."""
    g = torch.Generator().manual_seed(90)
    return tuple(torch.randn(s, generator=g) for s in SHAPES)


@functools.lru_cache(maxsize=None)
def grads():
    """grads()[step][tensor]: fp32 CPU, the AVERAGED gradient of that step."""
    g = torch.Generator().manual_seed(91)
    out = []
    for k, scale in enumerate(SCALES):
        step = []
        for s in SHAPES:
            mag = torch.rand(s, generator=g) * 1.5 + 0.5
            sign = (torch.randint(0, 2, s, generator=g) * 2 - 1).float()
            step.append(mag * sign * scale)
        if k == NAN_STEP:
            step[INF_AT[0]].view(-1)[INF_AT[1]] = float("inf")
        out.append(tuple(step))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def norms():
    """The float64 global norm of every step's averaged gradient."""
    return tuple(torch.sqrt(sum((t.double() ** 2).sum() for t in step)).item() for step in grads())


# Past the step kernels' grid cap (2048 blocks of 1024 elements): two tensors of 2048 * 1024 + 5 and 3 elements, 2097164 padded.  The
# vector tail of the first (one element behind 2097156) is reached in the second grid-stride trip, and the norm arrives as 2048
# partial sums, eight per thread of the step kernel's head.  Three steps of gradients built as grads() builds them; the norms are
# about 1.9e3, 5.7e4 and 1.9, so the clip acts on two steps and not on the third.  The parameters are built the same way,
# +-U[0.5, 2): Adam's L2 decay adds 0.1 * p to a clipped gradient of at most 0.006 per element, and among two million N(0, 1)
# parameters some would cancel it to within rounding, where m / sqrt(v) amplifies one float32 rounding to 1e-3 of the update;
# with |p| >= 0.5 the sum keeps the sign of p and the well-conditioned property of the short case carries over to this length.
LONG_SHAPES = [(2048 * 1024 + 5,), (3,)]
LONG_SCALES = [1.0, 30.0, 0.001]


def _signed_uniform(s, g):
    mag = torch.rand(s, generator=g) * 1.5 + 0.5
    sign = (torch.randint(0, 2, s, generator=g) * 2 - 1).float()
    return mag * sign


@functools.lru_cache(maxsize=None)
def long_params():
    g = torch.Generator().manual_seed(92)
    return tuple(_signed_uniform(s, g) for s in LONG_SHAPES)


@functools.lru_cache(maxsize=None)
def long_grads():
    g = torch.Generator().manual_seed(93)
    return tuple(tuple(_signed_uniform(s, g) * scale for s in LONG_SHAPES) for scale in LONG_SCALES)


def _optimizer(kind, ps, weight_decay):
    cls = {"SGD": torch.optim.SGD, "Adam": torch.optim.Adam, "AdamW": torch.optim.AdamW}[kind]
    return cls(ps, weight_decay=weight_decay, **HYPER[kind])


@functools.lru_cache(maxsize=None)
def replica(kind, dtype=torch.float64, fault=None, world=1, steps=len(SCALES), long=False):
    """The parameters after `steps` steps, one flat float64 vector (tensors in order, no padding).  world > 1: the replica sees
    the gradient summed over `world` equal ranks and averages it first, as the data-parallel trainer does; the only fault
    that can tell is 'summed_norm' (the norm taken of the sum instead of the average).  long: long_params() and long_grads()."""
    assert fault is None or fault == "summed_norm" or kind in FAULTS[fault], (kind, fault)
    start, gs = (long_params(), long_grads()) if long else (params(), grads())
    ps = [torch.nn.Parameter(p.to(dtype).clone()) for p in start]
    opt_kind = {"Adam": "AdamW", "AdamW": "Adam"}[kind] if fault == "decay_swapped" else kind
    wd = 0.0 if fault in ("no_decay", "coef_after_decay") else WEIGHT_DECAY
    opt = _optimizer(opt_kind, ps, wd)
    for step in gs[:steps]:
        summed = [g.to(dtype) * world for g in step]
        for p, g in zip(ps, summed):
            p.grad = g / world
        of = summed if fault == "summed_norm" else [p.grad for p in ps]
        norm = torch.sqrt(sum((g ** 2).sum() for g in of))
        if not torch.isfinite(norm):
            if fault == "skip_counts":
                for p in ps:
                    opt.state[p]["step"] += 1
            continue
        coef = torch.clamp(MAX_NORM / (norm + 1e-6), max=1.0)
        for p in ps:
            c = coef
            if fault == "per_tensor_norm":
                c = torch.clamp(MAX_NORM / (torch.sqrt((p.grad ** 2).sum()) + 1e-6), max=1.0)
            if fault == "coef_after_decay":
                p.grad = c * (p.grad + WEIGHT_DECAY * p.detach())
            elif fault != "no_clip":
                p.grad.mul_(c)
        opt.step()
    return torch.cat([p.detach().double().reshape(-1) for p in ps])


def rel_err(got, ref):
    """max|got - ref| / max|ref| over all parameters; NaN (a non-finite `got`) compares as outside every bound."""
    return ((got.double() - ref).abs().max() / ref.abs().max()).item()


def unpadded(flat, offsets, ps=None):
    """A flat optimizer buffer (tensors at `offsets`, padded to 4 elements) as the replica's vector; ps: params() unless given."""
    return torch.cat([flat[o:o + p.numel()].detach().double().cpu() for p, o in zip(ps or params(), offsets)])
