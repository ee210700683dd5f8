"""Time label smoothing at the shape of tools/time_weighted_loss.py: 128 x 5 = 640 caption rows, E = H = 512, V = 10000, L = 5, bf16
(the fused vocabulary projection + cross entropy, csrc/vocab_ce.hip).  In ONE process, alternating round by round: loss + backward
unsmoothed (the yardstick), with label_smoothing, and with label_smoothing and sequence_weight.  Prints per variant the minimum and
the median of the rounds (ms per call, HIP events around `reps` calls) and the smoothed / unsmoothed ratio; the same text goes to
the file named by the first argument (default profiles/time_label_smoothing.txt).  --label-smoothing sets eps (default 0.1)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from showtell_amd.rnn import RNN
from showtell_amd.train import synthetic_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "time_label_smoothing.txt"))
ap.add_argument("--label-smoothing", type=float, default=0.1)
args = ap.parse_args()
EPS = args.label_smoothing

E, H, V, L, B, S = 512, 512, 10000, 5, 128, 5
ROUNDS, REPS = 7, 10

torch.manual_seed(0)
m = RNN(E, H, V, L, dtype=torch.bfloat16).cuda().train()
_, cap, lens = synthetic_batch(B * S, V, seed=1, image_size=8)
feat = torch.randn(B * S, E, device="cuda", requires_grad=True)
adv = torch.randn(B * S, device="cuda")


def train(**kw):
    for p in m.parameters():
        p.grad = None
    m.loss(feat, cap, lens, **kw).backward()


variants = [("loss + backward, unsmoothed", lambda: train()),
            (f"loss + backward, label_smoothing={EPS:g}", lambda: train(label_smoothing=EPS)),
            ("  ... and sequence_weight", lambda: train(label_smoothing=EPS, sequence_weight=adv))]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


for _, fn in variants:          # warm-up: working copies, gradient buffers, the plan
    for _ in range(3):
        fn()
torch.cuda.synchronize()
ms = [[] for _ in variants]
for _ in range(ROUNDS):
    for i, (_, fn) in enumerate(variants):
        ms[i].append(timed(fn))
lines = [f"RNN bf16, {B} x {S} = {B * S} caption rows ({sum(lens)} tokens), E = H = {E}, V = {V}, L = {L}; {ROUNDS} alternating rounds of {REPS} calls, ms per call"]
for (name, _), t in zip(variants, ms):
    lines.append(f"{name:38s} min {min(t):.3f}  median {statistics.median(t):.3f}  max {max(t):.3f}   rounds: " + " ".join(f"{v:.3f}" for v in t))
lines.append(f"smoothed / unsmoothed: {min(ms[1]) / min(ms[0]):.4f} (minima), {statistics.median(ms[1]) / statistics.median(ms[0]):.4f} (medians)")
lines.append(f"smoothed and weighted / unsmoothed: {min(ms[2]) / min(ms[0]):.4f} (minima), {statistics.median(ms[2]) / statistics.median(ms[0]):.4f} (medians)")
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write(text)
