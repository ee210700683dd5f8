"""Time scheduled sampling at the benchmark's decoder shape: bf16 GRU, B = 128 captions, E = H = 512, V = 10000, L = 5 (bench.py),
loss + backward through the fused vocabulary projection + cross entropy.  In ONE process, alternating round by round: the plain
call (the yardstick), loss(scheduled_sampling = p) at p = 0, 0.25 and 1 (the roll-in and then the loss on the mixed inputs), and
loss(input_ids = fixed ids) alone (what the separate input ids cost without a roll-in).  Prints per variant the minimum and the
median of the rounds (ms per call, HIP events around `reps` calls) and the time each adds to the yardstick.

Then, in the same process, the roll-in itself beside ``sample``: st_rnn_sched_inputs over the captions (max(lens) - 1 steps) and
st_rnn_sample with one draw per image over as many steps, microseconds per step.

The same text goes to the file named by the first argument (default profiles/time_scheduled_sampling.txt)."""
import argparse
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?", default=None)
ap.add_argument("--rounds", type=int, default=9)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from showtell_amd.rnn import RNN
from showtell_amd.train import synthetic_batch

E, H, V, L, B = 512, 512, 10000, 5, 128
ROUNDS, REPS = args.rounds, 10

_, cap, lens = synthetic_batch(B, V, seed=1, image_size=8)
feat = torch.randn(B, E, device="cuda", requires_grad=True)
torch.manual_seed(0)
m = RNN(E, H, V, L, dtype=torch.bfloat16).cuda().train()
gen = torch.Generator(device="cuda")
gen.manual_seed(1)
with torch.no_grad():
    fixed_ids = m.scheduled_inputs(feat, cap, lens, 0.25, generator=gen)[0]


def train(**kw):
    for p in m.parameters():
        p.grad = None
    m.loss(feat, cap, lens, **kw).backward()


variants = [("plain", "loss(feat, cap, lens)", {}),
            ("p0", "scheduled_sampling = 0", dict(scheduled_sampling=0.0, ss_generator=gen)),
            ("p025", "scheduled_sampling = 0.25", dict(scheduled_sampling=0.25, ss_generator=gen)),
            ("p1", "scheduled_sampling = 1", dict(scheduled_sampling=1.0, ss_generator=gen)),
            ("ids", "input_ids = fixed ids (no roll-in)", dict(input_ids=fixed_ids))]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


for _, _, kw in variants:          # warm-up: working copies, gradient buffers, the plan
    for _ in range(3):
        train(**kw)
torch.cuda.synchronize()
ms = [[] for _ in variants]
for _ in range(ROUNDS):
    for i, (_, _, kw) in enumerate(variants):
        ms[i].append(timed(lambda: train(**kw)))
lines = [f"RNN bf16 GRU, {B} captions ({sum(lens)} tokens, longest {max(lens)}), E = H = {E}, V = {V}, L = {L}, loss + backward; {ROUNDS} alternating "
         f"rounds of {REPS} calls, ms per call"]
base_min, base_med = min(ms[0]), statistics.median(ms[0])
for (key, text, _), t in zip(variants, ms):
    lines.append(f"{key:6s} {text:36s} min {min(t):.3f}  median {statistics.median(t):.3f}  max {max(t):.3f}   "
                 f"added to plain: {1e3 * (min(t) - base_min):+.1f} us (minima) {1e3 * (statistics.median(t) - base_med):+.1f} us (medians)")
lines.append(f"plain: spread of the rounds (max - min) {1e3 * (max(ms[0]) - min(ms[0])):.1f} us")

# the roll-in beside sample, per step
steps = max(lens) - 1


def roll(p):
    with torch.no_grad():
        m.scheduled_inputs(feat, cap, lens, p, generator=gen)


def sample():
    with torch.no_grad():
        m.sample(feat, 1, max_length=steps, generator=gen)


loops = [("sample", f"sample(num_samples = 1, max_length = {steps})", sample), ("roll0", "scheduled_inputs(p = 0)", lambda: roll(0.0)),
         ("roll025", "scheduled_inputs(p = 0.25)", lambda: roll(0.25)), ("roll1", "scheduled_inputs(p = 1)", lambda: roll(1.0))]
for _, _, fn in loops:
    for _ in range(3):
        fn()
torch.cuda.synchronize()
us = [[] for _ in loops]
for _ in range(ROUNDS):
    for i, (_, _, fn) in enumerate(loops):
        us[i].append(1e3 * timed(fn) / steps)
lines.append(f"the loops alone, {B} rows, {steps} steps, us per step (Python call included)")
for (key, text, _), t in zip(loops, us):
    lines.append(f"{key:8s} {text:44s} min {min(t):.1f}  median {statistics.median(t):.1f}  max {max(t):.1f}")
text = "\n".join(lines) + "\n"
print(text, end="")
out = args.out or os.path.join(ROOT, "profiles", "time_scheduled_sampling.txt")
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as fh:
    fh.write(text)
