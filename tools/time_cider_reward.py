"""Time the CIDEr reward of the self-critical step on the host (evaluation.cider_reward) and on the device
(evaluation.cider_reward_device, st_cider_reward) at the benchmark's decoder shape: bf16 GRU, E = H = 512, V = 10000, L = 5,
B = 128 images, S = 5 samples of 25 tokens, five references of 8 to 15 words per image.  Everything in ONE process, in
alternating rounds (ROUNDS, default 9), medians and minima reported:

  reward, host     cider_reward on CPU copies of the samples and of the greedy captions: S + 1 cider_score calls, as the host path
                   of Trainer.step_self_critical makes them (host clock)
  reward, device   one .advantage(ids, lengths, 'greedy', greedy_ids) call: host clock around the call and a synchronisation, and
                   device events around REPS back-to-back calls (the launch itself; the table is the batch's own, as on the host)
  step, host       Trainer.step_self_critical (ResNet-101 + the GRU, as bench.py builds them) with cider_reward, ms per step,
  step, device     ... and with cider_reward_device (host clock around the step and a synchronisation)

The yardstick is the host path in the same process.  The text also goes to the file named by the first argument."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from showtell_amd import evaluation, optim
from showtell_amd.cnn import ResNet
from showtell_amd.rnn import CAP_MAX, RNN
from showtell_amd.train import Trainer

E = H = 512
V, L, B, S, END = 10000, 5, 128, 5, 2
ROUNDS = int(os.environ.get("ROUNDS", "9"))
REPS = 50


def inputs():
    """references, and samples that share n-grams with them: every sample is one of its image's references with a third of the
    words redrawn, continued with random words to CAP_MAX tokens or ended by <end>"""
    rng = np.random.RandomState(0)
    refs = [[[int(t) for t in rng.randint(4, V, size=rng.randint(8, 16))] for _ in range(5)] for _ in range(B)]
    ids = np.zeros((B, S, CAP_MAX), dtype=np.int64)
    for b in range(B):
        for s in range(S):
            r = list(refs[b][s])
            for i in rng.choice(len(r), size=len(r) // 3, replace=False):
                r[i] = int(rng.randint(4, V))
            r = r + [END] if s % 2 else r + [int(t) for t in rng.randint(4, V, size=CAP_MAX - len(r))]
            ids[b, s, :len(r)] = r
    ids = torch.from_numpy(ids)
    from showtell_amd.rnn import sample_lengths
    return refs, ids, sample_lengths(ids, END), ids[:, 0].clone()


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    refs, ids, lengths, greedy = inputs()
    host_fn = evaluation.cider_reward(refs, END)
    dev_fn = evaluation.cider_reward_device(refs, None, END)
    ids_d, len_d, greedy_d = ids.cuda(), lengths.cuda(), greedy.cuda()
    greedy_len = lengths[:, :1]

    def host_reward():
        ids_d.cpu(), len_d.cpu()                                                  # what the host path copies first
        host_fn(greedy.reshape(B, 1, -1), greedy_len), host_fn(ids, lengths)

    def device_reward():
        dev_fn.advantage(ids_d, len_d, "greedy", greedy_d, check_lengths=False)

    torch.manual_seed(0)
    cnn = ResNet(101, E, dtype=torch.bfloat16).cuda().train()
    rnn = RNN(E, H, V, L, dtype=torch.bfloat16).cuda().train()
    with torch.no_grad():
        rnn.linear.weight *= 12.0                                                 # as tools/time_sample.py: not a flat distribution
    tr = Trainer(cnn, rnn, optim.SGD(Trainer.trainable_params(cnn, rnn), lr=0.0, momentum=0.0))     # lr 0: every round the same model
    image = torch.randn(B, 3, 224, 224, device="cuda")
    u = torch.rand(B, S, CAP_MAX, device="cuda")
    calls = {"reward, host": lambda: clock(host_reward), "reward, device (call + sync)": lambda: clock(device_reward),
             "reward, device (events)": lambda: events(device_reward),
             "step, host reward": lambda: clock(lambda: tr.step_self_critical(image, host_fn, num_samples=S, uniforms=u)),
             "step, device reward": lambda: clock(lambda: tr.step_self_critical(image, dev_fn, num_samples=S, uniforms=u))}
    names = list(calls)
    for name in names:                                                            # warm-up: every call twice
        calls[name](), calls[name]()
    times = {name: [] for name in names}
    for r in range(ROUNDS):
        for name in (names if r % 2 == 0 else names[::-1]):                       # alternating order
            times[name].append(calls[name]())
    same = (dev_fn(ids_d, len_d).cpu() - host_fn(ids, lengths)).abs().max().item()
    lines = [f"CIDEr reward, B = {B}, S = {S} (+ the greedy caption), {CAP_MAX}-token samples, five references per image, batch df "
             f"(K = {dev_fn.table.keys.numel()} keys); step: ResNet-101 + bf16 GRU E = H = {E}, V = {V}, L = {L}; {ROUNDS} alternating "
             f"rounds, ms: median / min / max",
             f"device rewards against the host's on these inputs: max |d| {same:.2e} (mean reward {host_fn(ids, lengths).mean().item():.3f})"]
    for name in names:
        t = sorted(times[name])
        lines.append(f"  {name:30s} {statistics.median(t):10.4f} / {t[0]:10.4f} / {t[-1]:10.4f}")
    med = {name: statistics.median(times[name]) for name in names}
    lines.append(f"host / device, reward call: {med['reward, host'] / med['reward, device (call + sync)']:.0f} x (medians); "
                 f"step: {med['step, host reward']:.2f} -> {med['step, device reward']:.2f} ms, "
                 f"{med['step, host reward'] / med['step, device reward']:.1f} x")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
