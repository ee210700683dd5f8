"""The cases, weights and float64 oracle that tests/test_gpu_weighted_loss.py and tests/test_weighted_loss_inputs.py share.

A case is a decoder, a caption batch and signed weights (per sequence AND per token, both in [-1, 1]; they multiply).  The
oracle is R.rnn_forward / R.attn_forward in float64; the weighted loss  sum_r w_r * nll_r / N_tok  (+ the unweighted
doubly-stochastic term of the attention decoders) and its autograd are written here.  Every reference is computed once per
process (lru_cache) and handed out as is: callers do not modify it.

The bound on a weighted gradient is the project's relative bound in its linear form.  With w = w+ - w- (the positive and the
negative part), g(w) = g(w+) - g(w-) up to the unweighted term, and each half is an ordinary non-negatively weighted
cross-entropy gradient that the kernels deliver to `tol` of its own scale; so
    max|g_gpu(w) - g_ref(w)|  <=  tol * (max|g_ref(w+)| + max|g_ref(w-)|),
all three right-hand quantities from the oracle.  tol = 4e-2 for bf16 (`_rel` of tests/test_gpu_decoder.py), 1e-3 for fp32
(tests/test_gpu_config0.py).  The halves can cancel, which would leave the bound without power: the CPU test requires
max|g_ref(w)| >= 5 % of the right-hand scale for every parameter."""
import functools

import torch

from oracle import restatement as R
from tests._util import load_fixture

# name: (family, cell, dtype, E, H, V, L, B)
CASES = {
    "gru777": ("rnn", "gru", "bf16", 512, 512, 777, 2, 9),
    "lstm1500": ("rnn", "lstm", "bf16", 512, 512, 1500, 2, 33),
    "gru_fp32": ("rnn", "gru", "fp32", 64, 64, 200, 2, 16),
    "attn_fp32": ("attn", "gru", "fp32", None, None, None, None, None),     # tests/golden/attn_gru_small.npz
}
GRAD_TOL = {"bf16": 4e-2, "fp32": 1e-3}
# softmax is shift invariant: d(loss)/d(attn.full_att.bias) is analytically zero (tests/test_gpu_attention.py), so a bound
# relative to the oracle's value of it (rounding noise of float64) says nothing; it is held to the absolute 1e-5 used there
ZERO_GRADS = {"attn.full_att.bias": 1e-5}


def torch_dtype(case):
    return torch.bfloat16 if CASES[case][2] == "bf16" else torch.float32


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(params, feat, caption, lens, alpha_c) as fp32 CPU tensors; for bf16 cases already rounded to bf16-representable values,
    so that the kernels and the oracle see the same numbers."""
    family, cell, dt, E, H, V, L, B = CASES[case]
    if family == "attn":
        params, _, d = load_fixture("attn_gru_small.npz")
        return params, torch.from_numpy(d["feat"]), torch.from_numpy(d["caption"]), d["lens"].tolist(), float(d["alpha_c"])
    if dt == "bf16":        # the ragged shapes of test_fused_vocab_cross_entropy_matches_launch_chain_and_oracle
        params = R.init_decoder_params(E, H, V, L, cell, seed=5)
        cap, lens = R.synthetic_captions(B, V, seed=5, mean=7, std=2, lo=3, hi=11)
        feat = torch.randn(B, E, generator=torch.Generator().manual_seed(5))
        params = {k: v.bfloat16().float() for k, v in params.items()}
        feat = feat.bfloat16().float()
    else:
        params = R.init_decoder_params(E, H, V, L, cell, seed=3)
        cap, lens = R.synthetic_captions(B, V, seed=3, mean=8, std=2, lo=4, hi=12)
        feat = torch.randn(B, E, generator=torch.Generator().manual_seed(3))
    return params, feat, cap, lens, 0.0


@functools.lru_cache(maxsize=None)
def weights(case):
    """(sequence_weight (B,), token_weight (B, T)) fp32, uniform in [-1, 1]."""
    _, _, cap, _, _ = inputs(case)
    g = torch.Generator().manual_seed(17 + len(case))
    return torch.rand(cap.shape[0], generator=g) * 2 - 1, torch.rand(tuple(cap.shape), generator=g) * 2 - 1


def packed_weights(case):
    """The weight of every packed row, float64: pack_rows of sequence_weight[b] * token_weight[b, t]."""
    _, _, _, lens, _ = inputs(case)
    sw, tw = weights(case)
    return R.pack_rows(sw.double()[:, None] * tw.double(), lens)


def oracle_logits(case, params, feat, cap, lens):
    family, cell = CASES[case][:2]
    if family == "attn":
        return R.attn_forward(params, feat, cap, lens, cell)
    return R.rnn_forward(params, feat, cap, lens, cell), None


def weighted_loss(logits, alphas, target, w, alpha_c):
    """sum_r w_r * (logsumexp(x_r) - x_r[target_r]) / N_tok  (+ alpha_c * mean((1 - sum_t alpha)^2), unweighted)."""
    nll = torch.logsumexp(logits, 1) - logits.gather(1, target[:, None])[:, 0]
    loss = (w * nll).sum() / nll.shape[0]
    if alphas is not None:
        loss = loss + alpha_c * ((1.0 - alphas.sum(dim=1)) ** 2).mean()
    return loss


def oracle_grads(case, params, feat, cap, lens, w, alpha_c, feat_grad=True):
    """One float64 forward, three backward passes: {'loss', 'g', 'gp', 'gm'} for the weights w, max(w, 0), max(-w, 0); each g a
    dict over the parameters (and 'feat')."""
    po = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    fo = feat.double().clone().requires_grad_(feat_grad)
    logits, alphas = oracle_logits(case, po, fo, cap, lens)
    target = R.pack_rows(cap, lens)
    leaves = dict(po)
    if feat_grad:
        leaves["feat"] = fo
    out = {}
    for name, wk in (("g", w), ("gp", w.clamp(min=0)), ("gm", (-w).clamp(min=0))):
        loss = weighted_loss(logits, alphas, target, wk, alpha_c)
        gs = torch.autograd.grad(loss, list(leaves.values()), retain_graph=True, allow_unused=True)
        out[name] = {k: (torch.zeros_like(v) if g is None else g) for (k, v), g in zip(leaves.items(), gs)}
        if name == "g":
            out["loss"] = loss.item()
    return out


@functools.lru_cache(maxsize=None)
def reference(case):
    params, feat, cap, lens, alpha_c = inputs(case)
    return oracle_grads(case, params, feat, cap, lens, packed_weights(case), alpha_c, feat_grad=CASES[case][0] != "attn")


def grad_scale(ref, k):
    """The right-hand scale of the linear-form bound for parameter k."""
    return ref["gp"][k].abs().max().item() + ref["gm"][k].abs().max().item()


def assert_grads_within_linear_bound(got, ref, tol, what=""):
    """got: {name: tensor} from the kernels; ref: oracle_grads(..).  Prints every figure before it asserts."""
    worst = []
    for k, g in got.items():
        err = (g.detach().double().cpu() - ref["g"][k]).abs().max().item()
        if k in ZERO_GRADS:
            print(f"{what} {k}: max|g| {g.abs().max().item():.3e} (analytically zero, bound {ZERO_GRADS[k]:.0e})")
            worst.append((g.abs().max().item() / ZERO_GRADS[k], k))
            continue
        scale = grad_scale(ref, k)
        print(f"{what} {k}: err {err:.3e}  scale {scale:.3e}  ratio {err / scale:.3e}  (bound {tol:.0e})")
        worst.append((err / (tol * scale), k))
    bad = [(r, k) for r, k in worst if not r <= 1.0]
    assert not bad, f"{what}: outside the bound (error / bound, parameter): {bad}"
