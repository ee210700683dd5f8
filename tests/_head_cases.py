"""The inputs, the float64 oracle and the seeded faults that tests/test_head_inputs.py and tests/test_gpu_head.py share: the
encoder head y = BatchNorm1d(Linear(x)) of showtell_amd/head.py (csrc/head_optim.hip: st_linear_bn1d_forward / _backward).

Every case is the smallest (B, F, E) that still reaches its branch of the kernels:

  tiny        3,    8,   4   K is one vector; Bp = 8, so 5 of the 8 contraction rows of dW are padding; one partial 32-column
                             block; the smallest batch variance, where eps matters (B = 3: at B = 2 the train-mode dz is zero)
  odd        13,   64,  36   B % 8 = 5; E % 8 = 4, so dz rows are Ep = 40 apart; E % 32 = 4, a second block with 4 live lanes;
                             row groups with unequal trip counts
  single      1,  512, 256   eval only: captioning one image; split-K in both dtypes with M = 1
  split_edge 70,  512, 100   split-K in both dtypes; two 64-row transpose tiles with Bp = 72; E % 8 = 4 and E % 32 = 4
  long_k      9, 1000,  64   F % 256 != 0: the unsplit GEMM over a long K in both dtypes
  tall      257,  256,  32   five transpose row tiles, 33 rows per row group; fp32 is split, bf16 is not

The oracle is written out by hand (no nn.BatchNorm1d).  In float64 it is the reference; in float32 it is the replica that measures
the reference's own error; with round_dz it rounds dz to bf16 before dW and dbias, the one place where the bf16 kernels round
after their inputs; with one of FAULTS seeded it shows that the bounds can tell.  Everything is computed once per process
(lru_cache) and handed out as is: callers do not modify it."""
import functools
import math

import torch

from tests._util import _bf16

MOMENTUM, EPS = 0.01, 1e-5
# name: (B, F, E, modes)
CASES = {
    "tiny": (3, 8, 4, ("train", "eval")),
    "odd": (13, 64, 36, ("train", "eval")),
    "single": (1, 512, 256, ("eval",)),
    "split_edge": (70, 512, 100, ("train", "eval")),
    "long_k": (9, 1000, 64, ("train", "eval")),
    "tall": (257, 256, 32, ("train", "eval")),
}
DTYPES = ("float32", "bfloat16")                 # the kernels' compute dtype
ACCUMULATION_CASES = ("odd", "split_edge")
GRADS = ("dW", "dbias", "dgamma", "dbeta")       # linear.weight, linear.bias, bn.weight, bn.bias
TENSORS = ("y", "running_mean", "running_var") + GRADS

# max|got - ref| / max|ref| per tensor (errors() below).  From the reference alone, on a CPU:
# the float32 replica differs from the float64 oracle by at most 1.44e-6 (tiny, train, dW; then y 1.01e-6, dbias 5.9e-7, dgamma
# 5.8e-7, dbeta 1.5e-7, running_var 9.9e-8, running_mean 8.2e-8: the largest over all cases, modes and the two-step accumulation
# runs); ten times the largest leaves room for fused multiply-add, split-K atomics and another summation order.  In bf16 mode it
# also holds for y, the running statistics, dgamma and dbeta: they never pass through bf16 after the inputs.
BOUND_F32 = 1.4e-5
# the float64 replica that rounds dz to bf16 differs in dW by at most 2.87e-3 (tall, train; one bf16 rounding is 2^-9 = 1.95e-3)
# and in dbias by at most 2.45e-3 (split_edge, eval, two steps); four times the former, for dW and dbias in bf16 mode.
BOUND_BF16_DZ = 1.1e-2


def up8(v):
    return (v + 7) & ~7


def al256(v):
    return (v + 255) & ~255


def split_k(B, F, E, dtype):
    """st_linear_bn1d_forward's route: 8 K slices when F is a multiple of 8 k-blocks (64 wide in bf16, 32 in fp32)."""
    bk = 64 if dtype == "bfloat16" else 32
    return F % (8 * bk) == 0 and B * E <= 256 * 128 * 64


def workspace_bytes(B, F, E, dtype):
    """st_head_workspace_bytes: dz [B][Ep], dz^T [E][Bp] and x^T [F][Bp] in the compute dtype, each at a 256-byte boundary."""
    es = 2 if dtype == "bfloat16" else 4
    return al256(B * up8(E) * es) + al256(E * up8(B) * es) + al256(F * up8(B) * es)


@functools.lru_cache(maxsize=None)
def inputs(case, dtype):
    """fp32 CPU tensors: x, dy and a second batch x2, dy2; W, b, gamma, beta, running_mean, running_var; the non-zero starting
    gradients g0_*.  In bf16 mode x, x2 and W hold bf16 values (the same draws, rounded)."""
    B, F, E, _ = CASES[case]
    g = torch.Generator().manual_seed(4100 + list(CASES).index(case))
    d = {
        "x": torch.randn(B, F, generator=g).abs(),                        # pooled post-ReLU features
        "W": torch.randn(E, F, generator=g) * 0.05,                       # cnn.py:41
        "b": (torch.rand(E, generator=g) * 2 - 1) / math.sqrt(F),
        "gamma": torch.rand(E, generator=g) + 0.5,
        "beta": torch.randn(E, generator=g) * 0.1,
        "running_mean": torch.randn(E, generator=g) * 0.1,
        "running_var": torch.rand(E, generator=g) + 0.5,
        "dy": torch.randn(B, E, generator=g),
        "x2": torch.randn(B, F, generator=g).abs(),
        "dy2": torch.randn(B, E, generator=g),
        "g0_dW": torch.randn(E, F, generator=g),
        "g0_dbias": torch.randn(E, generator=g),
        "g0_dgamma": torch.randn(E, generator=g),
        "g0_dbeta": torch.randn(E, generator=g),
    }
    if dtype == "bfloat16":
        for k in ("x", "x2", "W"):
            d[k] = _bf16(d[k])
    return d


# fault: what it needs of (B, F, E, dtype, train); the two-step-only fault is listed apart
def _is_split(B, F, E, dtype, train):
    return split_k(B, F, E, dtype)


FAULTS = {
    "biased_running_var": lambda B, F, E, dtype, train: train,        # the biased variance written to running_var
    "momentum_swapped": lambda B, F, E, dtype, train: train,          # momentum and 1 - momentum swapped
    "eval_batch_stats": lambda B, F, E, dtype, train: not train,      # eval normalising with batch statistics
    "train_running_stats": lambda B, F, E, dtype, train: train,       # train normalising with running statistics
    "eps_dropped": lambda B, F, E, dtype, train: train,               # rstd = 1 / sqrt(var)
    "no_m1": lambda B, F, E, dtype, train: train,                     # the mean(dy) term dropped from the train dz
    "no_m2": lambda B, F, E, dtype, train: train,                     # the mean(dy * xhat) term dropped from the train dz
    "m1_m2_in_eval": lambda B, F, E, dtype, train: not train,         # both applied in eval
    "partial_block_zero": lambda B, F, E, dtype, train: E % 32 != 0,  # the last partial 32-column block left at zero
    "dz_stride_E": lambda B, F, E, dtype, train: up8(E) != E,         # dz written Ep apart, read back E apart
    "pad_row_copy": lambda B, F, E, dtype, train: B % 8 != 0,         # pad row B of dz^T and x^T holds row 0, not zeros
    "bias_per_slice": _is_split,                                      # the bias added by every split-K slice
    "slice_dropped": _is_split,                                       # one of the eight K slices missing
}
ACCUMULATION_FAULT = "overwrite_grads"                                # gradients written, not accumulated
# The cases whose row in the table above names the branch a fault lives in; everywhere else the fault is measured and printed
# but need not show.  biased_running_var moves running_var by momentum * var / B relative to running_var ~ 1, and var, the batch
# variance of z, grows with F (about 0.0025 * 0.36 * F): only the long K at a small B brings that well above 1e-5.  eps against
# var shows only where var is smallest.
FAULT_CASES = {
    "biased_running_var": ("long_k",),
    "eps_dropped": ("tiny",),
    "partial_block_zero": ("tiny", "odd", "split_edge"),
    "dz_stride_E": ("tiny", "odd", "split_edge"),
    "pad_row_copy": ("tiny", "odd", "split_edge", "long_k"),
    "bias_per_slice": ("single", "split_edge", "tall"),
    "slice_dropped": ("single", "split_edge", "tall"),
}


def fault_cases(fault):
    return FAULT_CASES.get(fault, tuple(CASES))


def oracle(p, x, dy, rm, rv, train, dtype=torch.float64, round_dz=False, fault=None):
    """One forward and backward of the head, written out.  p: W, b, gamma, beta; x [B][F], dy [B][E]; rm, rv the running
    statistics before the call.  Returns y, the running statistics after it, dz and the four gradients of sum(y * dy), in `dtype`."""
    W, b, gamma, beta = (p[k].to(dtype) for k in ("W", "b", "gamma", "beta"))
    x, dy, rm, rv = x.to(dtype), dy.to(dtype), rm.to(dtype), rv.to(dtype)
    B, F = x.shape
    E = W.shape[0]
    xs = x
    if fault == "slice_dropped":
        xs = x.clone()
        xs[:, 3 * (F // 8):4 * (F // 8)] = 0
    z = xs @ W.t() + (8 * b if fault == "bias_per_slice" else b)
    bmean = z.sum(0) / B
    dev = z - bmean
    ss = (dev * dev).sum(0)
    var_b, var_u = ss / B, (ss / (B - 1) if B > 1 else ss / B)
    use_batch = (train and fault != "train_running_stats") or (not train and fault == "eval_batch_stats")
    mean, var = (bmean, var_b) if use_batch else (rm, rv)
    rstd = 1 / torch.sqrt(var + (0.0 if fault == "eps_dropped" else EPS))
    rm_new, rv_new = rm.clone(), rv.clone()
    if train:
        keep, take = (MOMENTUM, 1 - MOMENTUM) if fault == "momentum_swapped" else (1 - MOMENTUM, MOMENTUM)
        rm_new = keep * rm + take * bmean
        rv_new = keep * rv + take * (var_b if fault == "biased_running_var" else var_u)
    xh = (z - mean) * rstd
    y = xh * gamma + beta
    dbeta, dgamma = dy.sum(0), (dy * xh).sum(0)
    if train or fault == "m1_m2_in_eval":
        m1 = 0 if fault == "no_m1" else dbeta / B
        m2 = 0 if fault == "no_m2" else dgamma / B
        dz = gamma * rstd * (dy - m1 - xh * m2)
    else:
        dz = gamma * rstd * dy
    if fault == "partial_block_zero":
        e0 = E // 32 * 32
        y, dz, dgamma, dbeta = y.clone(), dz.clone(), dgamma.clone(), dbeta.clone()
        y[:, e0:] = 0; dz[:, e0:] = 0; dgamma[e0:] = 0; dbeta[e0:] = 0
        rm_new[e0:] = rm[e0:]; rv_new[e0:] = rv[e0:]
    if round_dz:
        dz = dz.float().bfloat16().to(dtype)
    dz_read = dz
    if fault == "dz_stride_E":
        buf = torch.zeros(B * up8(E), dtype=dtype)
        buf.view(B, up8(E))[:, :E] = dz
        dz_read = buf[:B * E].view(B, E)
    dW = dz_read.t() @ x
    if fault == "pad_row_copy":
        dW = dW + torch.outer(dz_read[0], x[0])
    return {"y": y, "running_mean": rm_new, "running_var": rv_new, "dz": dz, "dW": dW, "dbias": dz_read.sum(0), "dgamma": dgamma, "dbeta": dbeta}


@functools.lru_cache(maxsize=None)
def run(case, dtype, train, replica=torch.float64, round_dz=False, fault=None, steps=1):
    """`steps` forwards and backwards (the second on x2, dy2) that start from the gradients g0 and accumulate, as the GPU test
    drives linear_bn1d.  Returns float64: y of the last call, the running statistics after it, the four gradients MINUS g0
    (accumulated and subtracted in the replica's dtype, as the comparison does), and dz_l1[e] = sum over calls and rows of |dz|."""
    p = inputs(case, dtype)
    rm, rv = p["running_mean"], p["running_var"]
    grads = {k: p["g0_" + k].to(replica).clone() for k in GRADS}
    l1 = 0
    for s in range(steps):
        o = oracle(p, p["x2" if s else "x"], p["dy2" if s else "dy"], rm, rv, train, replica, round_dz, None if fault == ACCUMULATION_FAULT else fault)
        rm, rv = o["running_mean"], o["running_var"]
        for k in GRADS:
            grads[k] = o[k].clone() if fault == ACCUMULATION_FAULT else grads[k] + o[k]
        l1 = l1 + o["dz"].abs().sum(0)
    out = {"y": o["y"], "running_mean": rm, "running_var": rv, "dz_l1": l1}
    out.update({k: grads[k] - p["g0_" + k].to(replica) for k in GRADS})
    return {k: v.double() for k, v in out.items()}


def errors(got, ref, train):
    """max|got - ref| / max|ref| for every tensor of TENSORS that `got` holds.  In train mode dbias is analytically zero and is
    measured against the terms that cancel in it: max|dbias| / max_e sum_b |dz[b, e]|.  NaN compares as outside every bound."""
    out = {}
    for k in TENSORS:
        if k not in got:
            continue
        g = got[k].detach().double().cpu()
        if k == "dbias" and train:
            out[k] = (g.abs().max() / ref["dz_l1"].max()).item()
        else:
            out[k] = ((g - ref[k]).abs().max() / ref[k].abs().max()).item()
    return out


def bounds(dtype):
    b = {k: BOUND_F32 for k in TENSORS}
    if dtype == "bfloat16":
        b["dW"] = b["dbias"] = BOUND_BF16_DZ
    return b


def outside(errs, dtype):
    """The tensors of `errs` that miss their bound."""
    b = bounds(dtype)
    return [k for k, e in errs.items() if not e <= b[k]]
