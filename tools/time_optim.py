"""Time the optimizer step at the benchmark's parameter count (19.18 M fp32 parameters with a bf16 shadow), in
ONE process, alternating round by round: Adam and SGD(momentum) plain (one launch, st_adam_step / st_sgd_step), with
max_grad_norm (st_grad_sumsq + st_*_step_ex), and with max_grad_norm + weight_decay + skip_nonfinite; and the sum-of-squares
launch alone.  Prints per variant the minimum and the median of the rounds (microseconds per step, HIP events around `reps`
steps) and the ratios to the plain step; the same text goes to the file named by the first argument (default
profiles/time_optim.txt)."""
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from showtell_amd import optim
from showtell_amd._lib import check, lib, ptr, stream

N = 19_180_000
ROUNDS, REPS = 7, 20
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "time_optim.txt")

gen = torch.Generator().manual_seed(0)
start = torch.randn(N, generator=gen) * 0.05
grad = (torch.randn(N, generator=gen) * 1e-3).cuda()           # norm about 4.4: max_grad_norm = 1 clips every step


def make(cls, **kw):
    opt = cls([torch.nn.Parameter(start.clone().cuda())], **kw)
    opt.flat_grad.copy_(grad)
    return opt


FULL = dict(max_grad_norm=1.0, weight_decay=0.01, skip_nonfinite=True)
opts = [("Adam plain", make(optim.Adam, lr=1e-4)),
        ("Adam max_grad_norm", make(optim.Adam, lr=1e-4, max_grad_norm=1.0)),
        ("Adam max_grad_norm + weight_decay + skip_nonfinite", make(optim.Adam, lr=1e-4, **FULL)),
        ("AdamW max_grad_norm + weight_decay + skip_nonfinite", make(optim.AdamW, lr=1e-4, **FULL)),
        ("SGD plain", make(optim.SGD, lr=0.01, momentum=0.9)),
        ("SGD max_grad_norm", make(optim.SGD, lr=0.01, momentum=0.9, max_grad_norm=1.0)),
        ("SGD max_grad_norm + weight_decay + skip_nonfinite", make(optim.SGD, lr=0.01, momentum=0.9, **FULL))]
partials = torch.empty(lib().st_grad_sumsq_max_parts(), device="cuda")
nparts = ctypes.c_int(0)


def sumsq():
    check(lib().st_grad_sumsq(ptr(grad), N, ptr(partials), ctypes.byref(nparts), stream()), "st_grad_sumsq")


variants = [(name, o.step) for name, o in opts] + [("st_grad_sumsq alone", sumsq)]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3


for _, fn in variants:
    for _ in range(3):
        fn()
torch.cuda.synchronize()
us = [[] for _ in variants]
for _ in range(ROUNDS):
    for i, (_, fn) in enumerate(variants):
        us[i].append(timed(fn))
for name, o in opts:
    assert torch.isfinite(o.flat).all() and (o.skipped_steps is None or int(o.skipped_steps) == 0), name
lines = [f"{N} fp32 parameters, bf16 shadow; {ROUNDS} alternating rounds of {REPS} steps, microseconds per step (host launch included)"]
for (name, _), t in zip(variants, us):
    lines.append(f"{name:52s} min {min(t):8.2f}  median {statistics.median(t):8.2f}  max {max(t):8.2f}   rounds: " + " ".join(f"{v:.1f}" for v in t))
for base, rows in ((0, (1, 2, 3)), (4, (5, 6))):
    for r in rows:
        lines.append(f"{variants[r][0]} / {variants[base][0]}: {min(us[r]) / min(us[base]):.4f} (minima), "
                     f"{statistics.median(us[r]) / statistics.median(us[base]):.4f} (medians)")
lines.append(f"st_grad_sumsq alone / Adam plain: {min(us[-1]) / min(us[0]):.4f} (minima), {statistics.median(us[-1]) / statistics.median(us[0]):.4f} (medians)")
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write(text)
