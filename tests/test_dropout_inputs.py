"""CPU checks of what tests/test_gpu_dropout.py compares against: the numpy replica of the dropout mask, the float64 oracle and
the power of the chosen cases against seeded faults (tests/_dropout_cases.py).

Known answers: the Philox4x32-10 vectors of the Random123 distribution (kat_vectors), which the replica must reproduce word for
word.  The C header's generator is the same few lines; the GPU file shows st_dropout_rows bit-equal to the replica.

Power: a GPU result within the bounds of the truth is only evidence if a wrong kernel would fall outside them.  For every case of
the GPU file, each fault of _dropout_cases.FAULTS that can touch the case must move at least one compared quantity (the loss, a
parameter gradient, feat.grad) by at least 10 x that quantity's bound.  This is a condition on the cases (their probabilities and
seeds), checked here so that it cannot silently stop holding."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from oracle import restatement as R
from tests import _dropout_cases as D
from tests._util import ROOT

KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_replica_reproduces_the_philox_known_answers(counter, key, want):
    got = D.philox4x32_10([np.array([c]) for c in counter], key)
    assert tuple(int(w[0]) for w in got) == want


def test_the_c_header_reproduces_the_known_answers_and_the_replicas_words():
    """csrc/dropout.h compiled for the host (it is a host and device header): the known answers, and drop_words / drop_key against the
    replica for a seed with both halves set, a late step, and the input site."""
    seed, step, site, rows, cols, p = (0xFEDCBA98 << 32) | 0x76543210, 123456, D.SITE_INPUT, 5, 16, 0.3
    lines = ['#include <stdio.h>', '#include "dropout.h"', 'int main() {']
    for counter, key, _ in KAT:
        lines.append('  { DropWords w = philox4x32_10(%uu, %uu, %uu, %uu, %uu, %uu); printf("%%u %%u %%u %%u\\n", w.w[0], w.w[1], w.w[2], w.w[3]); }'
                     % (counter + key))
    lines += ['  DropKey k = drop_key(%r, (long)%dULL, %d);' % (p, seed, step), '  printf("%u %a\\n", k.thr, (double)k.scale);',
              '  for (int r = 0; r < %d; ++r) for (int c4 = 0; c4 < %d; ++c4) { DropWords w = drop_words(k, %d, 7 + r, c4); '
              'printf("%%u %%u %%u %%u\\n", w.w[0], w.w[1], w.w[2], w.w[3]); }' % (rows, cols // 4, site), '  return 0;', '}']
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "kat.cpp"), os.path.join(td, "kat")
        open(src, "w").write("\n".join(lines) + "\n")
        subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "show-tell_amd", "csrc"), src, "-o", exe])
        out = subprocess.check_output([exe], text=True).splitlines()
    for (_, _, want), line in zip(KAT, out):
        assert tuple(map(int, line.split())) == want
    thr, scale = out[3].split()
    assert int(thr) == D.threshold(p) and float.fromhex(scale) == float(D.scale_of(p))
    got = np.array([list(map(int, l.split())) for l in out[4:]], dtype=np.uint32).reshape(rows, cols)
    assert np.array_equal(got, D.words(seed, step, site, rows, cols, row0=7))


def test_the_descriptor_mirror_has_the_headers_layout():
    """showtell_amd.dropout.DropoutDesc against st_dropout, by the check of tests/test_abi.py (dropout.py hands out the mirror of _lib)."""
    from showtell_amd.dropout import DropoutDesc
    from tests.test_abi import layout_errors
    assert layout_errors([(DropoutDesc, "st_dropout")]) == []
    assert ctypes.sizeof(DropoutDesc) == 56


def test_threshold_scale_and_value_rule():
    assert D.threshold(0.5) == 1 << 31 and D.threshold(0.0) == 0 and D.threshold(0.1) == 429496729
    assert D.scale_of(0.5) == np.float32(2.0) and D.scale_of(0.1) == np.float32(1.0 / 0.9)
    x = np.full((3, 8), -1.5, np.float32)
    y = D.dropout_rows(x, 0.5, 1, 0, 0)
    assert set(np.unique(y)) <= {np.float32(-3.0), np.float32(0.0)} and not np.signbit(y[y == 0]).any()      # dropped: +0
    # bf16: the product is formed in float32 and rounded to nearest even once
    xb = D.bf16_round(np.linspace(-2, 2, 64, dtype=np.float32).reshape(4, 16))
    yb = D.dropout_rows(xb, 0.1, 1, 0, 0, bf16=True)
    keep = D.keep_mask(1, 0, 0, 4, 16, 0.1)
    assert np.array_equal(yb[keep], D.bf16_round(xb[keep] * D.scale_of(0.1))) and (yb[~keep] == 0).all()
    assert np.array_equal(D.bf16_round(np.array([1.00390625, 1.01171875], np.float32)), np.array([1.0, 1.015625], np.float32))   # ties to even


def test_mask_is_a_function_of_the_packed_row_not_of_the_call():
    whole = D.words(99, 3, 1, 12, 24)
    assert np.array_equal(D.words(99, 3, 1, 7, 24, row0=5), whole[5:12])
    assert not np.array_equal(D.words(99, 4, 1, 12, 24), whole) and not np.array_equal(D.words(99, 3, 2, 12, 24), whole)
    assert not np.array_equal(D.words(99 + (1 << 32), 3, 1, 12, 24), whole)          # the high half of the seed keys the generator too


@pytest.mark.parametrize("p", [0.5, 0.1])
def test_keep_rate_is_binomial(p):
    keep = D.keep_mask(20240607, 0, 2, 70, 512, p)
    n = keep.size
    assert abs(keep.sum() - n * (1 - p)) <= 5 * np.sqrt(n * p * (1 - p))


@pytest.mark.parametrize("case", ["gru_fp32_all", "lstm_fp32_all", "gru_bf16_all", "attn_gru_fp32", "attn_lstm_fp32"])
def test_oracle_without_dropout_is_the_restatement(case):
    params, feat, cap, lens, alpha_c = D.inputs(case)
    po = {k: v.double() for k, v in params.items()}
    with torch.no_grad():
        if D.CASES[case][0] == "attn":
            got = D.attn_loss(case, po, feat.double(), cap, lens, alpha_c, dropout=False)
            want = R.attn_train_loss(po, feat.double(), cap, lens, alpha_c, D.CASES[case][1])
            assert torch.equal(got[2], want[2])
        else:
            got = D.rnn_loss(case, po, feat.double(), cap, lens, dropout=False)
            want = R.gru_train_loss(po, feat.double(), cap, lens, D.CASES[case][1])
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_cases_cover_what_the_kernels_branch_on():
    for case in D.RNN_CASES:
        _, _, dt, E, H, V, L, B, p, seed = D.CASES[case]
        lens = D.inputs(case)[3]
        bs = R.batch_sizes(lens)
        assert all(0 <= q < 1 for q in p) and any(p)
        if H != 512:
            assert B > 16 and bs[0] > 16 and any(a > b for a, b in zip(bs, bs[1:])) and lens[0] == 9 and lens[-1] == 1 and L == 3
        if dt == "fp32":
            assert E != H and H % 16 != 0 and H % 8 == 0
    assert D.CASES["gru_bf16_fused"][9] >> 63 == 1              # a seed whose top bit is set crosses the C ABI as a negative long
    assert len({D.CASES["gru_fp32_all"][8][i] for i in range(3)}) == 3


def _moved(case, fault, step=0):
    """The largest ratio (deviation of the faulty result, or of another step's draw) / (the quantity's bound) over the compared
    quantities."""
    loss_b, rel_b = D.bounds(case)
    l0, g0, _, _ = D.oracle(case)
    l1, g1, _, _ = D.oracle(case, step, fault)
    worst = abs(l1 - l0) / loss_b
    for k in g0:
        if k in D.ZERO_GRADS or (k == "feat" and D.CASES[case][0] == "attn"):
            continue
        worst = max(worst, D.rel(g1[k], g0[k]) / rel_b)
    return worst


@pytest.mark.parametrize("case", list(D.CASES))
def test_every_fault_moves_a_compared_quantity_by_ten_bounds(case):
    for fault in D.faults_of(case):
        assert _moved(case, fault) >= 10.0, (case, fault, _moved(case, fault))


@pytest.mark.parametrize("case", ["gru_fp32_all", "lstm_bf16_all", "gru_bf16_fused", "attn_gru_fp32"])
def test_next_step_is_another_draw(case):
    """the cases of the GPU file's reproducibility test: step 1 is as far from step 0 as a fault is from the truth"""
    assert D.oracle(case, 1)[0] != D.oracle(case, 0)[0]
    assert _moved(case, None, step=1) >= 10.0


def test_constructor_arguments_seed_and_state_dict():
    from showtell_amd.rnn import RNN
    from showtell_amd.rnn_attn import RNN_Attn
    with pytest.warns(UserWarning, match="num_layers greater than 1"):
        RNN(16, 16, 20, 1, dropout=0.3)
    for bad in (1.0, -0.1, float("nan"), "x"):
        with pytest.raises(ValueError):
            RNN(16, 16, 20, 2, dropout_out=bad)
        with pytest.raises(ValueError):
            RNN_Attn(16, 16, 16, 16, 20, 2, dropout_out=bad)
    m = RNN(16, 16, 20, 2, dropout=0.3, dropout_out=0.5)
    assert not any("drop" in k for k in m.state_dict())                      # state_dict keys stay the reference's
    assert m._dropout.seed == torch.initial_seed() & ((1 << 64) - 1)
    m.seed_dropout(5)
    assert (m._dropout.seed, m._dropout.step) == (5, 0)


def test_trainer_seeds_rank_r_with_seed_plus_r(monkeypatch):
    """Data-parallel replicas must draw different masks: the Trainer re-seeds the decoder with its seed + the process's rank (0 without
    torch.distributed) and zeroes the step counter, whatever the world size."""
    import types
    from showtell_amd import train
    from showtell_amd.rnn import RNN
    from showtell_amd.rnn_attn import RNN_Attn
    assert train.dropout_rank() == 0
    for rank in (0, 3):
        monkeypatch.setattr(train, "dropout_rank", lambda r=rank: r)
        for m in (RNN(16, 16, 20, 2, dropout=0.3), RNN_Attn(16, 16, 16, 16, 20, 2, dropout_out=0.5)):
            m.seed_dropout((1 << 64) - 2)
            m._dropout.step = 5
            assert m.dropout_seed == (1 << 64) - 2
            train.Trainer(None, m, types.SimpleNamespace(), world_size=1)
            assert m.dropout_seed == ((1 << 64) - 2 + rank) % (1 << 64) and m._dropout.step == 0      # 64 bits: the sum wraps

