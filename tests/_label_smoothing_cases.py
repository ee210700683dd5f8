"""The cases, float64 oracle, bounds and seeded faults that tests/test_gpu_label_smoothing.py and
tests/test_label_smoothing_inputs.py share.

The oracle is torch's own definition, F.cross_entropy(logits, target, label_smoothing=eps) in float64 on the logits of
oracle/restatement.py; reduction='none' times the row weights gives the weighted form (the divisor stays N_tok, the
doubly-stochastic term of the attention decoders stays unsmoothed and unweighted).  Every reference is computed once per
process (lru_cache) and handed out as is: callers do not modify it.

Cases: those of tests/_weighted_loss_cases.py and one tiny bf16 decoder with V = 130 -- its second 128-entry tile holds 2 valid
entries in wave 0 and three fully masked waves.  Inputs differ from that file's in one respect: `linear.bias` is raised by
BIAS_OFFSET.  At the seeded initial weights the logits are nearly flat around 0, so a row's mean logit is 1e-3 to 1e-2 and a
fault that mishandles it (a mean over the padded row length: 1504 for 1500) moves u = logsumexp - mean by little more than the
fp32 rounding of logsumexp; an offset of 1 makes the mean logit 1 and leaves softmax, nll, u and every gradient what they were
(shift invariance).  tests/test_label_smoothing_inputs.py shows the faults that this makes visible.

Bounds (none comes from the code under test):
  u rows      4 x the float32-against-float64 difference of u computed on the CPU from the oracle's logits rounded to fp32
              (`u_floor`): what fp32 arithmetic costs on these very rows.
  gradients   the linear form of tests/_weighted_loss_cases.py: tol * (max|g_ref(w+)| + max|g_ref(w-)|), tol 4e-2 (bf16) / 1e-3
              (fp32), every quantity from the smoothed float64 oracle.
  dlogits     |d_eps - (d0 + eps * gw * (onehot - 1/V))| <= 2^-8 * (|d0| + |expected|) for bf16 output (two roundings of half an
              ulp, relative 2^-9 each, doubled), 2^-22 * (..) for fp32 output."""
import functools

import torch
import torch.nn.functional as F

from oracle import restatement as R
from tests import _weighted_loss_cases as W

# name: (family, cell, dtype, E, H, V, L, B)
CASES = {**W.CASES, "gru130": ("rnn", "gru", "bf16", 512, 512, 130, 1, 5)}
# (case, ST_FUSED_CE): gru777 also on the bf16 launch chain
ROUTES = [("gru777", "1"), ("gru777", "0"), ("lstm1500", "1"), ("gru130", "1"), ("gru_fp32", "1"), ("attn_fp32", "1")]
EPS = {"bf16": 0.3, "fp32": 0.1}            # see the module docstring of tests/test_label_smoothing_inputs.py
GRAD_TOL = W.GRAD_TOL
ZERO_GRADS = W.ZERO_GRADS
BIAS_OFFSET = 1.0
TILE = 128                                  # vocabulary entries per workgroup of csrc/vocab_ce.hip
DLOGITS_REL = {"bf16": 2.0 ** -8, "fp32": 2.0 ** -22}
LIN_WEIGHTS = (0.0, 0.5, -0.5, 1.0, -1.0, 2.0)


def dtype_name(case):
    return CASES[case][2]


def torch_dtype(case):
    return torch.bfloat16 if dtype_name(case) == "bf16" else torch.float32


def eps_of(case):
    return EPS[dtype_name(case)]


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(params, feat, caption, lens, alpha_c) as fp32 CPU tensors, bf16-representable for the bf16 cases; linear.bias raised by
    BIAS_OFFSET (and rounded again where the case is bf16)."""
    family, cell, dt, E, H, V, L, B = CASES[case]
    if case in W.CASES:
        params, feat, cap, lens, alpha_c = W.inputs(case)
        params = {k: v.clone() for k, v in params.items()}
    else:
        params = R.init_decoder_params(E, H, V, L, cell, seed=7)
        cap, lens = R.synthetic_captions(B, V, seed=7, mean=5, std=2, lo=2, hi=8)
        feat = torch.randn(B, E, generator=torch.Generator().manual_seed(7)).bfloat16().float()
        params = {k: v.bfloat16().float() for k, v in params.items()}
        alpha_c = 0.0
    bias = params["linear.bias"] + BIAS_OFFSET
    params["linear.bias"] = bias.bfloat16().float() if dt == "bf16" else bias
    return params, feat, cap, lens, alpha_c


def vocab(case):
    return inputs(case)[0]["linear.bias"].shape[0]


def ldd_of(case):
    """Row length of dlogits: V rounded up to 8 (every case is below the 2048 entries where the decoder rounds to 512)."""
    return (vocab(case) + 7) // 8 * 8


@functools.lru_cache(maxsize=None)
def weights(case):
    """(sequence_weight (B,), token_weight (B, T)) fp32, uniform in [-1, 1]: the recipe of tests/_weighted_loss_cases.py."""
    cap = inputs(case)[2]
    g = torch.Generator().manual_seed(17 + len(case))
    return torch.rand(cap.shape[0], generator=g) * 2 - 1, torch.rand(tuple(cap.shape), generator=g) * 2 - 1


def packed_weights(case):
    sw, tw = weights(case)
    return R.pack_rows(sw.double()[:, None] * tw.double(), inputs(case)[3])


def target_of(case):
    _, _, cap, lens, _ = inputs(case)
    return R.pack_rows(cap, lens)


def lin_weights(n):
    """Row weights from LIN_WEIGHTS, every value present."""
    idx = torch.randint(0, len(LIN_WEIGHTS), (n,), generator=torch.Generator().manual_seed(29))
    idx[:len(LIN_WEIGHTS)] = torch.arange(len(LIN_WEIGHTS))
    return torch.tensor(LIN_WEIGHTS)[idx]


def oracle_logits(case, params, feat, cap, lens):
    family, cell = CASES[case][:2]
    if family == "attn":
        return R.attn_forward(params, feat, cap, lens, cell)
    return R.rnn_forward(params, feat, cap, lens, cell), None


def smoothed_loss(logits, alphas, target, w, alpha_c, eps):
    """sum_r w_r * CE_eps(x_r, t_r) / N_tok (+ alpha_c * mean((1 - sum_t alpha)^2), unsmoothed and unweighted)."""
    per_row = F.cross_entropy(logits, target, reduction="none", label_smoothing=eps)
    loss = (w * per_row).sum() / per_row.shape[0]
    if alphas is not None:
        loss = loss + alpha_c * ((1.0 - alphas.sum(dim=1)) ** 2).mean()
    return loss


def oracle_grads(case, w, eps):
    """One float64 forward, three backward passes: {'loss', 'g', 'gp', 'gm'} for the weights w, max(w, 0), max(-w, 0)."""
    params, feat, cap, lens, alpha_c = inputs(case)
    feat_grad = CASES[case][0] != "attn"
    po = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    fo = feat.double().clone().requires_grad_(feat_grad)
    logits, alphas = oracle_logits(case, po, fo, cap, lens)
    target = R.pack_rows(cap, lens)
    leaves = dict(po)
    if feat_grad:
        leaves["feat"] = fo
    out = {}
    for name, wk in (("g", w), ("gp", w.clamp(min=0)), ("gm", (-w).clamp(min=0))):
        loss = smoothed_loss(logits, alphas, target, wk, alpha_c, eps)
        gs = torch.autograd.grad(loss, list(leaves.values()), retain_graph=True, allow_unused=True)
        out[name] = {k: (torch.zeros_like(v) if g is None else g) for (k, v), g in zip(leaves.items(), gs)}
        if name == "g":
            out["loss"] = loss.item()
    return out


@functools.lru_cache(maxsize=None)
def reference(case, weighted, smoothed=True):
    """The oracle for the case's eps (smoothed=False: eps = 0, the fault 'smoothing dropped in the backward pass')."""
    w = packed_weights(case) if weighted else torch.ones(len(target_of(case)), dtype=torch.float64)
    return oracle_grads(case, w, eps_of(case) if smoothed else 0.0)


grad_scale = W.grad_scale
assert_grads_within_linear_bound = W.assert_grads_within_linear_bound


# ---- u = logsumexp - mean of the valid logits, per row ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def oracle_rows(case):
    """The float64 oracle's logits rounded to fp32 (what a kernel can hold at best), as float64 (N_tok, V)."""
    params, feat, cap, lens, _ = inputs(case)
    with torch.no_grad():
        logits, _ = oracle_logits(case, {k: v.double() for k, v in params.items()}, feat.double(), cap, lens)
    return logits.float().double()


def u_of(x):
    """logsumexp(x_r) - mean(x_r) in the dtype of x."""
    return torch.logsumexp(x, 1) - x.mean(1)


def nll_of(x, target):
    return torch.logsumexp(x, 1) - x.gather(1, target[:, None])[:, 0]


@functools.lru_cache(maxsize=None)
def u_floor(case):
    """max_r |u_r in fp32 arithmetic - u_r in float64|, both from the same fp32 logits (the oracle's), on the CPU."""
    x = oracle_rows(case)
    return (u_of(x.float()).double() - u_of(x)).abs().max().item()


def u_bound(case):
    return 4.0 * u_floor(case)


def u_faults(case):
    """{name: per-row u} of seeded faults of the forward pass, float64, from the oracle's rows.
    'masked entries counted': the last tile's lanes past V enter the sum with what the fused kernel's accumulators hold there,
    the product with the clamped weight row V - 1 and no bias.  'tile j dropped': the sum misses one 128-entry tile."""
    x, V, ldd = oracle_rows(case), vocab(case), ldd_of(case)
    bias = inputs(case)[0]["linear.bias"].double()
    lse, s = torch.logsumexp(x, 1), x.sum(1)
    out = {"nll for u": nll_of(x, target_of(case))}
    if ldd != V:
        out["mean over ldd"] = lse - s / ldd
    ntile = (V + TILE - 1) // TILE
    if ntile * TILE != V:
        out["masked entries counted"] = lse - (s + (ntile * TILE - V) * (x[:, V - 1] - bias[V - 1])) / V
    for j in range(ntile):
        out[f"tile {j} dropped"] = lse - (s - x[:, j * TILE:(j + 1) * TILE].sum(1)) / V
    return out


# ---- dlogits rows: the kernels' two roundings on the CPU -------------------------------------------------------------------

def dlogits_bound(case, d0, expected):
    return DLOGITS_REL[dtype_name(case)] * (d0.abs() + expected.abs())


def dlogits_expected(case, d0, gw, target, eps):
    """d0 + eps * gw * (onehot - 1/V) in float64 from the unsmoothed rows d0 (n, ldd): the pad columns stay d0's zeros."""
    V = vocab(case)
    corr = torch.zeros_like(d0)
    corr[:, :V] = -1.0 / V
    corr[torch.arange(d0.shape[0]), target] += 1.0
    return d0 + eps * gw[:, None] * corr


def dlogits_model(case, gw, keep, unif, pad=0.0):
    """(n, ldd) rows as the kernels form them, on the CPU: p = exp(x - lse) in fp32 from the oracle's fp32 logits,
    d = (p - (keep * onehot + unif)) * gw in fp32, rounded to the output dtype; pad columns hold `pad` * gw.  Returned float64.
    keep = 1, unif = 0: the unsmoothed rows."""
    x = oracle_rows(case).float()
    n, V = x.shape
    p = torch.exp(x - torch.logsumexp(x, 1, keepdim=True))
    sub = torch.full_like(p, unif)
    sub[torch.arange(n), target_of(case)] += keep
    d = torch.zeros(n, ldd_of(case))
    d[:, :V] = (p - sub) * gw.float()[:, None]
    d[:, V:] = pad * gw.float()[:, None]
    return d.to(torch_dtype(case)).double()
