"""Time nucleus (top-p) sampling against the sampler without it: bf16 GRU at the benchmark's decoder shape (E = H = 512,
V = 10000, L = 5), B = 128 images as tools/time_sample.py, 1 and 5 samples per image, 25 steps.  Six calls of RNN.sample, in
alternating rounds in one process (host clock around whole calls, each ended by a synchronisation; end_id = -1, so no row
ever finishes and every step draws every row):

  yardstick   top_k = 0 through ANOTHER build of the library: ST_YARDSTICK_LIB names a libshowtell_hip.so built from the
              commit to compare with (without it the tool times the other five alone)
  p=1         top_p = 1.0: the nucleus off, the launch the yardstick makes
  p=0.9       top_p = 0.9        p=0.5   top_p = 0.5
  k20 p=0.9   top_k = 20 and top_p = 0.9
  k32         top_k = 32 alone: the existing truncation's price, next to which the nucleus rows are read

Reported: microseconds per step, median / min / max, the difference of each median to the first row's and to p=1, and the
spread of each call's own rounds."""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from showtell_amd import _lib
from showtell_amd.rnn import CAP_MAX, RNN

E = H = 512
V, L, B = 10000, 5, 128
ROUNDS = int(os.environ.get("ROUNDS", "9"))
CALLS = {"p=1": dict(top_p=1.0), "p=0.9": dict(top_p=0.9), "p=0.5": dict(top_p=0.5), "k20 p=0.9": dict(top_k=20, top_p=0.9),
         "k32": dict(top_k=32)}


def _other_build(path):
    """the entry points of another build of the library, bound like _lib's own (the ones it has)"""
    cdll = C.CDLL(path)
    b = _lib._Bound.__new__(_lib._Bound)
    b.st_last_error = cdll.st_last_error
    b.st_last_error.argtypes, b.st_last_error.restype = [], C.c_char_p
    for name, (args, res) in _lib._SIGS.items():
        if hasattr(cdll, name):
            fn = getattr(cdll, name)
            fn.argtypes, fn.restype = args, res
            setattr(b, name, fn)
    return b


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    ours = _lib.lib()
    yard = _other_build(os.environ["ST_YARDSTICK_LIB"]) if os.environ.get("ST_YARDSTICK_LIB") else None
    torch.manual_seed(0)
    m = RNN(E, H, V, L, dtype=torch.bfloat16).cuda().eval()
    with torch.no_grad():
        m.linear.weight *= 12.0                                                   # as tools/time_sample.py: not a flat distribution
    feat = torch.randn(B, E, device="cuda")
    names = (["yardstick"] if yard else []) + list(CALLS)
    for S in (1, 5):
        u = torch.rand(B, S, CAP_MAX, device="cuda")

        def run(name):
            _lib._lib = yard if name == "yardstick" else ours
            try:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m.sample(feat, num_samples=S, end_id=-1, uniforms=u, **CALLS.get(name, {}))
                torch.cuda.synchronize()
                return time.perf_counter() - t0
            finally:
                _lib._lib = ours

        for name in names * 3:                                                    # warm-up: every call three times
            run(name)
        times = {name: [] for name in names}
        for r in range(ROUNDS):
            for name in (names if r % 2 == 0 else names[::-1]):                   # alternating order
                times[name].append(run(name))
        print(f"plain GRU, bf16, B={B} num_samples={S} ({B * S} rows), {CAP_MAX} steps, {ROUNDS} alternating rounds; us per step: "
              f"median / min / max, against the first row, against p=1")
        med = {name: sorted(ts)[len(ts) // 2] for name, ts in times.items()}
        for name in names:
            ts = sorted(times[name])
            us = lambda x: x / CAP_MAX * 1e6
            print(f"  {name:10s} {us(med[name]):8.2f} / {us(ts[0]):8.2f} / {us(ts[-1]):8.2f}    {us(med[name] - med[names[0]]):+7.2f}"
                  f"    {us(med[name] - med['p=1']):+7.2f}   (spread of its rounds {us(ts[-1] - ts[0]):.2f})")


if __name__ == "__main__":
    main()
