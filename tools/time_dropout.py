"""Time the decoders' dropout at the benchmark's decoder shape: bf16 GRU, B = 128 captions, E = H = 512, V = 10000, L = 5 (bench.py),
loss + backward through the fused vocabulary projection + cross entropy.  In ONE process, alternating round by round: the module
built without the dropout arguments (the yardstick), every p = 0 in train(), and each site on alone and all three together.  Prints
per variant the minimum and the median of the rounds (ms per call, HIP events around `reps` calls) and the time each adds to the
yardstick; the same text goes to the file named by the first argument (default profiles/time_dropout.txt).

  --only NAME --calls N   no timing: N calls of one variant after one warm-up call, for a kernel trace (rocprofv3 --kernel-trace -- python
                          tools/time_dropout.py --only layer --calls 5); the difference of two variants' launch counts over N is what
                          a site adds per call
  --plain-only            the yardstick alone, built without the new constructor arguments: the same loop on a checkout from before
                          the feature (--root DIR names the checkout whose package is timed; default: this one)"""
import argparse
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?", default=None)
ap.add_argument("--only", default=None)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--rounds", type=int, default=9)
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
sys.path.insert(0, ROOT)
import torch

from showtell_amd.rnn import RNN
from showtell_amd.train import synthetic_batch

E, H, V, L, B = 512, 512, 10000, 5, 128
ROUNDS, REPS = args.rounds, 10
P = {"in": dict(dropout_in=0.2), "layer": dict(dropout=0.3), "out": dict(dropout_out=0.5),
     "all": dict(dropout_in=0.2, dropout=0.3, dropout_out=0.5)}

_, cap, lens = synthetic_batch(B, V, seed=1, image_size=8)
feat = torch.randn(B, E, device="cuda", requires_grad=True)


def module(**kw):
    torch.manual_seed(0)
    return RNN(E, H, V, L, dtype=torch.bfloat16, **kw).cuda().train()


def train(m):
    for p in m.parameters():
        p.grad = None
    m.loss(feat, cap, lens).backward()


names = [("plain", "built without the arguments", {})]
if not args.plain_only:
    names += [("zero", "every p = 0, train()", dict(dropout=0.0, dropout_in=0.0, dropout_out=0.0)),
              ("in", "dropout_in = 0.2", P["in"]), ("layer", "dropout = 0.3 (between layers)", P["layer"]),
              ("out", "dropout_out = 0.5", P["out"]), ("all", "all three sites", P["all"])]
if args.only:
    names = [n for n in names if n[0] == args.only]
    assert names, f"unknown variant {args.only}"
variants = [(key, text, module(**kw)) for key, text, kw in names]

if args.only:
    m = variants[0][2]
    train(m)
    torch.cuda.synchronize()
    for _ in range(args.calls):
        train(m)
    torch.cuda.synchronize()
    print(f"{args.only}: 1 warm-up call + {args.calls} calls of loss + backward")
    sys.exit(0)


def timed(m):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        train(m)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


for _, _, m in variants:          # warm-up: working copies, gradient buffers, the plan
    for _ in range(3):
        train(m)
torch.cuda.synchronize()
ms = [[] for _ in variants]
for _ in range(ROUNDS):
    for i, (_, _, m) in enumerate(variants):
        ms[i].append(timed(m))
lines = [f"RNN bf16 GRU, {B} captions ({sum(lens)} tokens), E = H = {E}, V = {V}, L = {L}, loss + backward; {ROUNDS} alternating rounds of "
         f"{REPS} calls, ms per call"]
base_min, base_med = min(ms[0]), statistics.median(ms[0])
for (key, text, _), t in zip(variants, ms):
    lines.append(f"{key:6s} {text:32s} min {min(t):.3f}  median {statistics.median(t):.3f}  max {max(t):.3f}   "
                 f"added to plain: {1e3 * (min(t) - base_min):+.1f} us (minima) {1e3 * (statistics.median(t) - base_med):+.1f} us (medians)")
lines.append(f"plain: spread of the rounds (max - min) {1e3 * (max(ms[0]) - min(ms[0])):.1f} us")
text = "\n".join(lines) + "\n"
print(text, end="")
out = args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "time_dropout.txt")
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as fh:
    fh.write(text)
