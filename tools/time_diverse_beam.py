"""Time diverse (group) beam search against the single beam: bf16, the benchmark's decoder shape (E = H = 512, V = 10000, L = 5,
B = 256 images, W = 6, max_length = 25), plain GRU and attention GRU (F = 2048, P = 49, A = 512).  In alternating rounds in one
process (host clock around whole searches, each of which ends in a device-to-host copy):

  G=1            beam_search(...) with num_beam_groups=1: the single beam (st_softmax_topk + st_beam_select with one group)
  G=2, 3, 6      num_beam_groups=G, diversity_penalty=0.5: the same st_beam_select launch over G groups
  G=2, 3, 6 all  the same with min_length=5, no_repeat_ngram_size=3, suppress_tokens=[<pad>, <start>, <unk>]
  all            the three constraints with one group: what the rows above are to be compared with
  rec G=1, 6     plain GRU only: beam.beam_search_records, the device loop and its copies without the host-side replay of the
                 hypotheses (which runs once per group); compared with each other they show the selection launch alone

The yardstick is the single-beam search of ANOTHER build of the library, measured in the same rounds: ST_YARDSTICK_LIB names a
libshowtell_hip.so built from the commit to compare with (one that exports this tree's set of entry points: another is refused; without it the tool times its own calls alone).  A random decoder
never emits <end>, so every group stays live for all 25 iterations: the most work a search can do."""
import ctypes as C
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from oracle import restatement as R
from showtell_amd import _lib
from showtell_amd.beam import beam_search_records
from showtell_amd.rnn import RNN
from showtell_amd.rnn_attn import RNN_Attn

E = H = A = 512
Fd, P, V, L, B, W, T = 2048, 49, 10000, 5, 256, 6, 25
ROUNDS = int(os.environ.get("ROUNDS", "9"))
ALL = dict(min_length=5, no_repeat_ngram_size=3, suppress_tokens=[0, 1, 3])
CALLS = {"G=1": dict(num_beam_groups=1)}
CALLS.update({f"G={g}": dict(num_beam_groups=g, diversity_penalty=0.5) for g in (2, 3, 6)})
CALLS["all"] = dict(ALL)
CALLS.update({f"G={g} all": dict(num_beam_groups=g, diversity_penalty=0.5, **ALL) for g in (2, 3, 6)})
RECORDS = {"rec G=1": dict(num_beam_groups=1), "rec G=6": dict(num_beam_groups=6, diversity_penalty=0.5)}


def _other_build(path):
    """the entry points of another build of the library, bound like _lib's own.  It gets this tree's signatures, so a build that
    exports another set of st_ entry points (an ABI before or after this one) is refused before anything is launched"""
    def exports(p):
        out = subprocess.check_output(["nm", "-D", "--defined-only", p], text=True)
        return {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("st_")}
    theirs, mine = exports(path), exports(_lib.LIB_PATH)
    if theirs != mine:
        sys.exit(f"ST_YARDSTICK_LIB={path} exports other entry points than this tree's library "
                 f"(only there: {sorted(theirs - mine)}, only here: {sorted(mine - theirs)}): its calls cannot be bound with this tree's signatures")
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
    g = torch.Generator().manual_seed(31)
    plain = RNN(E, H, V, L, dtype=torch.bfloat16)
    plain.load_state_dict(R.init_decoder_params(E, H, V, L, "gru", seed=31))
    attn = RNN_Attn(E, Fd, A, H, V, L, dtype=torch.bfloat16)
    attn.load_state_dict(R.init_decoder_params(E, H, V, L, "gru", seed=31, attn=dict(F=Fd, A=A)))
    models = {"plain GRU": (plain.cuda().eval(), torch.randn(B, E, generator=g).cuda()),
              "attention GRU": (attn.cuda().eval(), torch.randn(B, Fd, P, generator=g).abs().cuda())}
    for tag, (m, feat) in models.items():
        names = (["yardstick"] if yard else []) + list(CALLS) + (list(RECORDS) if m is plain else [])

        def run(name):
            _lib._lib = yard if name == "yardstick" else ours
            try:
                t0 = time.perf_counter()
                if name in RECORDS:
                    beam_search_records(m, feat, W, T, **RECORDS[name])
                else:
                    m.beam_search(feat, beam_width=W, num_hypotheses=1, max_length=T, **CALLS.get(name, {}))
                torch.cuda.synchronize()
                return time.perf_counter() - t0
            finally:
                _lib._lib = ours

        for name in names * 2:                                                    # warm-up: every call twice
            run(name)
        times = {name: [] for name in names}
        for r in range(ROUNDS):
            for name in (names if r % 2 == 0 else names[::-1]):                   # alternating order
                times[name].append(run(name))
        print(f"{tag}, bf16, B={B} W={W} max_length={T}, {ROUNDS} alternating rounds; ms per search: median / min / max, "
              f"and us per iteration against the first row (rows with constraints: against `all`, `rec` rows: against `rec G=1`)")
        med = {name: sorted(ts)[len(ts) // 2] for name, ts in times.items()}
        for name in names:
            ts = sorted(times[name])
            base = med["all"] if name.endswith(" all") else med["rec G=1"] if name in RECORDS else med[names[0]]
            print(f"  {name:10s} {med[name] * 1e3:8.3f} / {ts[0] * 1e3:8.3f} / {ts[-1] * 1e3:8.3f}    {(med[name] - base) / T * 1e6:+7.2f} us/iteration"
                  f"   (spread of its rounds {(ts[-1] - ts[0]) / T * 1e6:.2f} us/iteration)")


if __name__ == "__main__":
    main()
