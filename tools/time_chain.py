"""Time the bf16 greedy launch chain alone (ST_DECODE_PIPE=0: no pipelined decoder) at the BASELINE decoder shape (B = 128,
E = H = 512, V = 10000, L = 5): microseconds per token step of RNN.sentence_index, five rounds of N calls (argument, default 50)
in one process.  The quiet counterpart of the last line of tools/time_sample.py, for A/B runs of library variants."""
import os, sys
os.environ["ST_DECODE_PIPE"] = "0"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from showtell_amd.rnn import RNN
torch.manual_seed(0)
m = RNN(512, 512, 10000, 5, dtype=torch.bfloat16).cuda().eval()
with torch.no_grad():
    m.linear.weight *= 12.0
feat = torch.randn(128, 512, device="cuda")
n = int(sys.argv[1]) if len(sys.argv) > 1 else 50
for _ in range(5):
    m.sentence_index(feat)
torch.cuda.synchronize()
res = []
for rep in range(5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        m.sentence_index(feat)
    e1.record(); torch.cuda.synchronize()
    res.append(e0.elapsed_time(e1) / n / 25 * 1e3)
print("chain us/step x5:", " ".join(f"{r:.2f}" for r in res))
