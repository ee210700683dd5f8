"""Time a bf16 beam search of the attention decoder: B = 256 images, W = 5, max_length = 25, with the config-3 decoder
(E = H = A = 512, F = 2048, P = 49, V = 10000, L = 5) at config-5's batch.  Prints captions/s and us per iteration (host
clock around whole searches that end in a device synchronise, after warm-up) beside the algorithmic work of one iteration."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from oracle import restatement as R
from showtell_amd.rnn_attn import RNN_Attn

E = H = A = 512
Fd, P, V, L, B, W, T = 2048, 49, 10000, 5, 256, 5, 25
N_RUNS = int(os.environ.get("N_RUNS", "10"))

assert torch.cuda.is_available(), "needs a GPU"
params = R.init_decoder_params(E, H, V, L, "gru", seed=31, attn=dict(F=Fd, A=A))
m = RNN_Attn(E, Fd, A, H, V, L, dtype=torch.bfloat16)
m.load_state_dict(params)
m = m.cuda().eval()
feat = torch.randn(B, Fd, P, generator=torch.Generator().manual_seed(31)).abs().cuda()


def run():
    return m.beam_search(feat, beam_width=W, num_hypotheses=1, max_length=T)   # ends in a device-to-host copy


for _ in range(3):
    run()
torch.cuda.synchronize()
times = []
for _ in range(N_RUNS):
    t0 = time.perf_counter()
    run()
    torch.cuda.synchronize()
    times.append(time.perf_counter() - t0)
times.sort()
med = times[len(times) // 2]
n = B * W
weights = sum(v.numel() for k, v in params.items() if "weight" in k and not k.startswith(("attn.encoder_att", "init_", "embeddings.")))   # GEMM operands of one iteration
flop = 2 * n * weights
feat_mb = B * P * (Fd + A) * 2 / 1e6                                         # feat + att1 (bf16), read once per iteration
print(f"attn beam bf16 B={B} W={W} T={T}: {B / med:.1f} captions/s, {med / T * 1e6:.1f} us/iteration "
      f"(median of {N_RUNS}, min {times[0] / T * 1e6:.1f}); per iteration: {weights / 1e6:.1f} M decoder weights "
      f"({weights * 2 / 1e6:.1f} MB bf16), {flop / 1e9:.1f} GFLOP, {feat_mb:.1f} MB of features; "
      f"compute floor {flop / 2.5e15 * 1e6:.1f} us at 2.5 PFLOP/s")
