"""Time st_rnn_backward alone at the bench shape (L = 5, B = 128, E = H = 512, V = 10000, bf16, the bench's caption lengths):
HIP events around 20 calls after 5 warm-ups, for the fused pull route and for ST_BPTT_FUSED=0 in the same process.
usage: python tools/time_bptt.py [gru|lstm]"""
import ctypes as C
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from showtell_amd._lib import ST_BF16, check, lib
from showtell_amd.rnn import RNN, _cp, _stream
from showtell_amd.rnn_lstm import RNN as RNN_LSTM
from showtell_amd.seq import plan_for
from showtell_amd.train import synthetic_batch

cell = sys.argv[1] if len(sys.argv) > 1 else "gru"
E, H, V, L, B = 512, 512, 10000, 5, 128
torch.manual_seed(1)
m = (RNN if cell == "gru" else RNN_LSTM)(E, H, V, L, dtype=torch.bfloat16).cuda().train()
_, caption, lens = synthetic_batch(B, V, seed=1, device="cuda", image_size=8)
plan = plan_for(lens, caption.device)
caption = caption.contiguous()
seq = plan.c_struct(caption)
prm, keep = m._c_params()
grads, keep2 = m._c_grads()
n, Vp = plan.ntok, lib().st_rnn_vocab_ld(V)
nbytes = lib().st_rnn_workspace_bytes(C.byref(prm), C.byref(seq))
ws = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
feat = torch.randn(B, E, device="cuda").bfloat16()
targets = torch.empty(n, device="cuda", dtype=torch.long)
check(lib().st_rnn_forward(C.byref(prm), C.byref(seq), _cp(feat), _cp(ws), nbytes, None, ST_BF16, Vp, _cp(targets), 1, None, None, _stream()),
      "st_rnn_forward")
dlog = (torch.randn(n, Vp, device="cuda") / n).bfloat16()
dlog[:, V:] = 0
dfeat = torch.empty(B, E, device="cuda", dtype=torch.float32)


def backward():
    check(lib().st_rnn_backward(C.byref(prm), C.byref(grads), C.byref(seq), _cp(dlog), Vp, _cp(ws), nbytes, _cp(dfeat), None, None,
                                _stream()), "st_rnn_backward")


def timed(warm=5, calls=20):
    for _ in range(warm):
        backward()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        backward()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


print(f"st_rnn_backward {cell} bf16 L={L} B={B} H={H} V={V}, {n} tokens, {plan.T} steps, {plan.T + L - 1} diagonals")
for fused in ("1", "0", "1", "0"):
    os.environ["ST_BPTT_FUSED"] = fused
    print(f"ST_BPTT_FUSED={fused}: {timed() * 1e3:.1f} us per call")
