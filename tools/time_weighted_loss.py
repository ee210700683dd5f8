"""Time the weighted loss at the self-critical shape: B = 128 images x S = 5 samples = 640 caption rows, E = H = 512, V = 10000,
L = 5, bf16 (the fused vocabulary projection + cross entropy, csrc/vocab_ce.hip).  In ONE process, alternating round by round:
loss + backward without weights, loss + backward with sequence_weight, and token_logp.  Prints per variant the minimum and
the median of the rounds (ms per call, HIP events around `reps` calls) and the weighted / unweighted ratio; the same text goes
to the file named by the first argument (default profiles/time_weighted_loss.txt)."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from showtell_amd.rnn import RNN
from showtell_amd.train import synthetic_batch

E, H, V, L, B, S = 512, 512, 10000, 5, 128, 5
ROUNDS, REPS = 7, 10
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "time_weighted_loss.txt")

torch.manual_seed(0)
m = RNN(E, H, V, L, dtype=torch.bfloat16).cuda().train()
_, cap, lens = synthetic_batch(B * S, V, seed=1, image_size=8)
feat = torch.randn(B * S, E, device="cuda", requires_grad=True)
adv = torch.randn(B * S, device="cuda")


def train(**kw):
    for p in m.parameters():
        p.grad = None
    m.loss(feat, cap, lens, **kw).backward()


variants = [("loss + backward, no weights", lambda: train()),
            ("loss + backward, sequence_weight", lambda: train(sequence_weight=adv)),
            ("token_logp", lambda: m.token_logp(feat, cap, lens))]


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
    lines.append(f"{name:34s} min {min(t):.3f}  median {statistics.median(t):.3f}  max {max(t):.3f}   rounds: " + " ".join(f"{v:.3f}" for v in t))
lines.append(f"weighted / unweighted: {min(ms[1]) / min(ms[0]):.4f} (minima), {statistics.median(ms[1]) / statistics.median(ms[0]):.4f} (medians)")
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    fh.write(text)
