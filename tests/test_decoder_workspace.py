"""Workspace layout of the decoder entry points (host-only: the planners read sizes, never a pointer).

tests/golden/decoder_workspace_bytes.json holds what every st_*_workspace_bytes planner of the recurrent decoders (and
st_rnn_vocab_ld) returned for the table below, recorded from the library before the planners were moved onto the shared
arena of csrc/decoder_host.h; the planners must reproduce every byte count.  The st_attn_beam_workspace_bytes keys that name
max_length, keep_paths and G hold what the separate planners of the constrained and the diverse search returned before the
one planner with st_beam_opts replaced them (keep_paths0 at max_length 64: those planners kept no paths there).
`python tests/test_decoder_workspace.py` rewrites the fixture from the library -- for an intended layout change only."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests._util import GOLDEN  # noqa: E402

FIXTURE = os.path.join(GOLDEN, "decoder_workspace_bytes.json")


def _bench_lens(B, seed):
    """Caption lengths of the benchmark's synthetic minibatch (train.synthetic_batch draws them first from this stream)."""
    rng = np.random.RandomState(seed)
    lens = np.clip(np.rint(rng.normal(12.5, 2.5, size=B)), 6, 25).astype(np.int64)
    return [int(v) for v in np.sort(lens)[::-1]]


RAGGED = [6] * 3 + [5] * 13 + [4] + [3] * 16 + [2] * 4        # batch sizes 37, 37, 33, 17, 16, 3
LONG = [70, 65]                                               # B = 2: ntok = 135 > B * P for P = 49 and P = 64

# name -> (E, H, L, V, lens); the plain decoder's layer-0 input is E wide
RNN_SHAPES = {
    "bench": (512, 512, 5, 10000, _bench_lens(128, 1)),      # pipe-eligible (bf16, E = H = 512)
    "narrow": (16, 40, 2, 50, RAGGED),                       # not pipe-eligible, nothing a multiple of a tile
    "v2047": (64, 64, 1, 2047, RAGGED),                      # the two branches of st_rnn_vocab_ld
    "v2049": (64, 64, 1, 2049, RAGGED),
    "deep8": (32, 32, 8, 50, RAGGED),                        # ST_MAX_LAYERS: the per-layer terms of the planners
}
# name -> (E, H, L, V, F, A, P, lens); Np = up8(max(ntok, B * P))
ATTN_SHAPES = {
    "bench_p49": (512, 512, 5, 10000, 2048, 512, 49, _bench_lens(64, 5)),    # ntok < B * P
    "bench_p64": (512, 512, 5, 10000, 2048, 512, 64, _bench_lens(64, 5)),
    "long_p49": (16, 40, 2, 50, 16, 16, 49, LONG),                           # ntok > B * P
    "long_p64": (16, 40, 2, 50, 16, 16, 64, LONG),
    "narrow_p4": (16, 40, 2, 50, 16, 16, 4, RAGGED),
    "deep8_p10": (32, 32, 8, 50, 48, 40, 10, RAGGED),
}
VOCAB_LD = (50, 2040, 2047, 2048, 2049, 10000)
BEAM_WIDTHS = (1, 8)
BEAM_LENGTHS = (14, 63, 64)                                   # 63: the longest search that keeps paths (ST_BEAM_MAX_HIST = 64)
CELLS = ("gru", "lstm")
DTYPES = ("f32", "bf16")


def _seq(lens):
    from showtell_amd import _lib
    T = lens[0]
    bs = (C.c_int * T)(*[sum(1 for v in lens if v > t) for t in range(T)])
    return _lib.PackedSeq(len(lens), T, sum(lens), T, bs, None, None, None, None)


def _rnn_params(cell, dtype, E, in0, H, L, V):
    from showtell_amd import _lib
    p = _lib.RnnParams()
    p.cell = _lib.ST_CELL_GRU if cell == "gru" else _lib.ST_CELL_LSTM
    p.dtype = _lib.ST_BF16 if dtype == "bf16" else _lib.ST_F32
    p.L, p.in0, p.H, p.V, p.E = L, in0, H, V, E
    return p


def table():
    """{case id: byte count} from the built library, in a fixed order."""
    from showtell_amd import _lib
    lib = _lib.lib()
    out = {}
    for V in VOCAB_LD:
        out["st_rnn_vocab_ld/V%d" % V] = lib.st_rnn_vocab_ld(V)
    for cell in CELLS:
        for dtype in DTYPES:
            for name, (E, H, L, V, lens) in RNN_SHAPES.items():
                p, s, B = _rnn_params(cell, dtype, E, E, H, L, V), _seq(lens), len(lens)
                tag = "/%s/%s/%s" % (name, cell, dtype)
                out["st_rnn_workspace_bytes" + tag] = lib.st_rnn_workspace_bytes(C.byref(p), C.byref(s))
                out["st_rnn_fused_loss_bytes" + tag] = lib.st_rnn_fused_loss_bytes(C.byref(p), C.byref(s))
                out["st_rnn_greedy_workspace_bytes" + tag] = lib.st_rnn_greedy_workspace_bytes(C.byref(p), B)
                out["st_rnn_sample_workspace_bytes" + tag] = lib.st_rnn_sample_workspace_bytes(C.byref(p), B)
            for name, (E, H, L, V, F, A, P, lens) in ATTN_SHAPES.items():
                p, s, B = _lib.AttnParams(), _seq(lens), len(lens)
                p.rnn = _rnn_params(cell, dtype, E, 2 * E, H, L, V)
                p.F, p.A, p.P = F, A, P
                tag = "/%s/%s/%s" % (name, cell, dtype)
                out["st_attn_workspace_bytes" + tag] = lib.st_attn_workspace_bytes(C.byref(p), C.byref(s))
                out["st_attn_greedy_workspace_bytes" + tag] = lib.st_attn_greedy_workspace_bytes(C.byref(p), B)
                out["st_attn_sample_workspace_bytes" + tag] = lib.st_attn_sample_workspace_bytes(C.byref(p), B)
                for W in BEAM_WIDTHS:
                    out["st_attn_beam_workspace_bytes%s/W%d" % (tag, W)] = plain = lib.st_attn_beam_workspace_bytes(C.byref(p), B, W, 14, None, None)
                    for T in BEAM_LENGTHS:
                        keep = int(T + 1 <= 64)
                        for G in sorted({1, W}):
                            o, off = _lib.BeamOpts(0, 0, None, 0, keep, G, 0.0), C.c_size_t(77)
                            key = "st_attn_beam_workspace_bytes%s/W%d/max_length%d/keep_paths%d/G%d" % (tag, W, T, keep, G)
                            out[key] = lib.st_attn_beam_workspace_bytes(C.byref(p), B, W, T, C.byref(o), C.byref(off))
                            # the last fringe's paths: buffer T & 1 of the two that follow the plain plan, each padded to 256 bytes
                            assert off.value == (plain + (T & 1) * ((B * W * (T + 1) * 4 + 255) // 256 * 256) if keep else 0), key
                        assert lib.st_attn_beam_workspace_bytes(C.byref(p), B, W, T, None, C.byref(off)) == plain and off.value == 0
    return out


def test_table_covers_both_sides_of_every_branch():
    """The shapes above sit where the planners branch; a fixture that missed a side would pin nothing there."""
    ntok = lambda lens: sum(lens)
    assert [sum(1 for v in RAGGED if v > t) for t in range(RAGGED[0])] == [37, 37, 33, 17, 16, 3]
    for name in ("bench_p49", "bench_p64", "narrow_p4"):
        E, H, L, V, F, A, P, lens = ATTN_SHAPES[name]
        assert ntok(lens) < len(lens) * P, name
    for name in ("long_p49", "long_p64"):
        E, H, L, V, F, A, P, lens = ATTN_SHAPES[name]
        assert ntok(lens) > len(lens) * P, name
    assert any(V < 2048 for V in VOCAB_LD) and any(V >= 2048 for V in VOCAB_LD)


def test_planners_reproduce_the_recorded_byte_counts():
    want = json.load(open(FIXTURE))
    got = table()
    assert sorted(got) == sorted(want)
    assert all(v > 0 for v in got.values()), [k for k, v in got.items() if v <= 0]
    bad = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not bad, bad


def test_pipelined_decoder_bytes_only_where_it_is_eligible():
    """The bf16 E = H = 512 greedy workspace carries the pipelined decoder's buffers; no other table entry does (the fp32
    workspace of the same shape has every launch-chain buffer at least as large, so it would otherwise be the bigger one)."""
    got = table()
    for cell in CELLS:
        assert got["st_rnn_greedy_workspace_bytes/bench/%s/bf16" % cell] > got["st_rnn_greedy_workspace_bytes/bench/%s/f32" % cell]
        assert got["st_rnn_greedy_workspace_bytes/narrow/%s/bf16" % cell] <= got["st_rnn_greedy_workspace_bytes/narrow/%s/f32" % cell]


if __name__ == "__main__":
    with open(FIXTURE, "w") as f:
        json.dump(table(), f, indent=1)
        f.write("\n")
    print("rewrote", FIXTURE)
