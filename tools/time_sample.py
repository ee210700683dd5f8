"""Time caption sampling at the BASELINE decoder shape (B = 128, E = H = 512, V = 10000, L = 5, bf16): microseconds per token
step of RNN.sample with 1 and 5 samples per image, and, in the same process, of the greedy launch chain (ST_DECODE_PIPE=0:
the route the sampling chain is built from; the sampling chain writes the fp32 logits every step, the greedy one does not)."""
import sys, os
os.environ["ST_DECODE_PIPE"] = "0"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from showtell_amd.rnn import RNN, CAP_MAX
E, H, V, L, B = 512, 512, 10000, 5, 128
torch.manual_seed(0)
m = RNN(E, H, V, L, dtype=torch.bfloat16).cuda().eval()
with torch.no_grad():
    m.linear.weight *= 12.0
feat = torch.randn(B, E, device="cuda")


def timed(fn, n=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


for S, k in ((1, 0), (5, 0), (1, 5), (5, 5)):
    u = torch.rand(B, S, CAP_MAX, device="cuda")
    ms = timed(lambda: m.sample(feat, num_samples=S, top_k=k, end_id=-1, uniforms=u))       # end_id -1: no row ever finishes
    print(f"sample bf16 B={B} num_samples={S} top_k={k}: {ms:.3f} ms / {CAP_MAX} steps = {ms / CAP_MAX * 1e3:.1f} us/step; "
          f"{B * S / ms * 1e3:.0f} captions/s")
ms = timed(lambda: m.sentence_index(feat))
print(f"greedy launch chain (ST_DECODE_PIPE=0) bf16 B={B}: {ms:.3f} ms / {CAP_MAX} steps = {ms / CAP_MAX * 1e3:.1f} us/step")
