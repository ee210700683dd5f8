"""Constrained beam search without a GPU: the inputs of test_gpu_beam_constraints.py have the power to fail a wrong kernel
(asserted from the float64 oracle's own constrained free run), the plain-Python ban rule against a brute-force enumeration,
seeded faults of that rule against the record walk, length-penalised ranking on hand-built records, argument validation."""
import numpy as np
import pytest
import torch

from tests import _beam_constraints_cases as K
from tests._beam_constraints_cases import END, START, T
from tests._beam_oracle import StepOracle, as_recorded, check_records

# the cases of test_gpu_beam_constraints.py, once per decoder (fp32 and bf16 share the parameters): (kind, cell, W, B, V)
DECODERS = {"plain-gru": ("plain", "gru", 4, 24, 600), "plain-lstm": ("plain", "lstm", 4, 24, 600), "plain-gru-w8": ("plain", "gru", 8, 9, 2056),
            "attn-gru": ("attn", "gru", 5, 13, 600), "attn-lstm": ("attn", "lstm", 5, 13, 600)}
# the constraint set on which the decoder's hypothesis lengths spread and length_penalty = 1 re-ranks: the combined set, except
# for the plain LSTM, whose combined-set hypotheses have nearly the same cost per word, so that length_penalty = 1 re-ranks none;
# test_gpu_beam_constraints.py ranks each decoder's hypotheses on the combined set and on this one
LP_SET = {"plain-gru": "all", "plain-lstm": "min6", "plain-gru-w8": "all", "attn-gru": "all", "attn-lstm": "all"}
NLL_ABS = 4 * 2.5e-6          # the record walk's bound on float64 records: 4 x the largest fp32 floor of test_gpu_beam_constraints

_RUNS = {}


def _run(name, cname):
    if (name, cname) not in _RUNS:
        kind, cell, W, B, vocab = DECODERS[name]
        orc = StepOracle(kind, cell, K.decoder_params(kind, cell, vocab, cname), K.features(kind, B), W, storage=False)
        _RUNS[(name, cname)] = (orc, K.free_run(orc, K.CONSTRAINTS[cname]))
    return _RUNS[(name, cname)]


def _first(rec, a=0.0):
    from showtell_amd.beam import replay_hypotheses
    hyp = replay_hypotheses(rec["tok"], rec["cost"].astype(np.float32), rec["par"], rec["end"], 1, length_penalty=a)
    return [tuple(h[0][0]) if h else None for h in hyp]


@pytest.mark.parametrize("cname", list(K.CONSTRAINTS))
@pytest.mark.parametrize("name", list(DECODERS))
def test_every_constraint_set_bites_on_its_inputs(name, cname):
    """Bite share: the share of live (iteration, slot) rows in which at least one of the unconstrained top W entries is banned,
    at least 0.15; on at least a quarter of those rows the ban set holds more than 5 % of the probability mass, so that a kernel
    that renormalised over the unbanned set moves the step cost by more than -log(0.95) = 0.05 nats, far beyond its bound."""
    _, rec = _run(name, cname)
    live, top = rec["live"], rec["top_banned"] & rec["live"]
    bite = top.sum() / live.sum()
    heavy = ((rec["mass_banned"] > 0.05) & top).sum() / max(1, top.sum())
    print(f"MEASURE {name} {cname}: bite share {bite:.2f}, of which with > 5 % banned mass {heavy:.2f}, live rows {live.sum()}")
    assert live.sum() >= 100 and bite >= 0.15 and heavy >= 0.25


@pytest.mark.parametrize("name", list(DECODERS))
def test_hypothesis_lengths_spread_and_the_length_penalty_reranks(name):
    _, rec = _run(name, LP_SET[name])
    h0, h1 = _first(rec), _first(rec, 1.0)
    lens = sorted({len(h) for h in h0 if h})
    changed = sum(a != b for a, b in zip(h0, h1))
    print(f"MEASURE {name} {LP_SET[name]}: first-hypothesis lengths {lens}, length_penalty = 1 changes {changed} of {len(h0)}")
    assert len(lens) >= 3 and changed >= len(h0) / 4


def test_ban_rule_against_brute_force():
    rng = np.random.default_rng(5)
    seen = 0
    for _ in range(400):
        t = int(rng.integers(0, 20))
        path = [START] + rng.integers(0, 5, t).tolist()                  # five words: every n-gram size repeats
        g, m = int(rng.integers(0, 5)), int(rng.integers(0, 8))
        sup = rng.integers(0, 12, int(rng.integers(0, 4))).tolist() or None
        want = K.banned_brute_force(path, 12, m, g, sup)
        assert {v for v in K.banned_tokens(path, m, g, sup) if v < 12} == want, (path, g, m, sup)
        seen += bool(want - set(sup or ()) - {END})
    assert seen >= 100                                                    # n-gram bans occur in at least a quarter of the draws
    assert K.banned_tokens([1, 7, 8, 7], g=2) == {8} and K.banned_tokens([1, 7, 8, 7], g=3) == set()
    assert K.banned_tokens([1, 7, 8, 7, 8], g=3) == {7} and K.banned_tokens([1, 7], g=1) == {1, 7}
    assert K.banned_tokens([1, 4, 4], g=2) == {4} and K.banned_tokens([1], 1) == {END} and K.banned_tokens([1, 3], 1) == set()


# ---- seeded faults: a Python mirror of the kernel's rule, broken on purpose; the record walk must catch each ------------------

def _mirror(path, m, g, sup, lo=0, hi=0, tail_shift=0, dg=0, skip_root=False, end_le=False):
    """st_beam_ban_topk's rule as the kernel computes it (one test per start i of an earlier n-gram), with the faults"""
    if skip_root:
        path = path[1:]
    n, t = len(path), len(path) - 1 + int(skip_root)
    g = g - dg if g else 0
    out = set(sup or ())
    if t < m or (end_le and t <= m):
        out.add(END)
    if g >= 1 and n:
        for i in range(lo, n - g + 1 - hi):
            if all(0 <= n - g + 1 + q - tail_shift < n and path[i + q] == path[n - g + 1 + q - tail_shift] for q in range(g - 1)):
                out.add(path[i + g - 1])
    return out


FAULTS = {                                                                # name -> (constraint set, free_run arguments)
    "window starts one late": ("g2s", dict(rule=lambda p, m, g, s: _mirror(p, m, g, s, lo=1))),
    "window ends one early": ("g2", dict(rule=lambda p, m, g, s: _mirror(p, m, g, s, hi=1))),
    "suffix one token back": ("g3", dict(rule=lambda p, m, g, s: _mirror(p, m, g, s, tail_shift=1))),
    "g - 1 for g": ("g3", dict(rule=lambda p, m, g, s: _mirror(p, m, g, s, dg=1))),
    "g + 1 for g": ("g2", dict(rule=lambda p, m, g, s: _mirror(p, m, g, s, dg=-1))),
    "s_0 left out": ("g1s", dict(rule=lambda p, m, g, s: _mirror(p, m, g, s, skip_root=True))),
    "t <= m for t < m": ("min6", dict(rule=lambda p, m, g, s: _mirror(p, m, g, s, end_le=True))),
    "bans after the top-k cut": ("sup5", dict(after_cut=True)),
    "sum over the unbanned entries": ("sup5", dict(renormalise=True)),
    "history of the slot, not of the parent": ("g2", dict(own_slot_paths=True)),
}


def test_the_mirror_without_faults_is_the_rule():
    rng = np.random.default_rng(6)
    for _ in range(300):
        path = [START] + rng.integers(0, 5, int(rng.integers(0, 20))).tolist()
        g, m = int(rng.integers(0, 5)), int(rng.integers(0, 8))
        assert _mirror(path, m, g, None) == K.banned_tokens(path, m, g, None)


ROOT_FAULTS = ("s_0 left out", "window starts one late")     # both concern the n-gram that begins with <start>: run on every decoder


@pytest.mark.parametrize("name,fault", [("plain-lstm", f) for f in FAULTS if f not in ROOT_FAULTS] + [(n, f) for n in DECODERS for f in ROOT_FAULTS])
def test_seeded_faults_are_caught_by_the_record_walk(name, fault):
    """each fault runs the float64 oracle's own search with the broken rule on the inputs of a GPU case (the same decoder, images
    and constraint set as test_gpu_beam_constraints.py walks); the walk of its records, the checks of that file, must fail, and
    passes on the unbroken search.  The two faults at the root of the path run on every decoder's g1s / g2s inputs, where <start>
    is wanted again: the attention search seeds and inherits its paths in code of its own."""
    cname, kw = FAULTS[fault]
    orc, rec = _run(name, cname)
    cons = K.CONSTRAINTS[cname]
    check_records(as_recorded(rec), orc, NLL_ABS, f"{name} {cname} unbroken", cons)
    with pytest.raises(AssertionError):
        check_records(as_recorded(K.free_run(orc, cons, **kw)), orc, NLL_ABS, f"{name} {cname} {fault}", cons)


# ---- length-penalised ranking ------------------------------------------------------------------------------------------

def _hand_records():
    """one image, W = 2, T = 6: hypotheses A, B, C, D harvested at iterations 2, 3, 4 and 5 with costs 2.0, 2.4, 4.0 and 3.0"""
    Tn, W = 6, 2
    tok = np.zeros((Tn + 1, 1, W), np.int64); cost = np.full((Tn + 1, 1, W), np.inf, np.float32)
    par = np.full((Tn + 1, 1, W), -1, np.int32); end = np.zeros((Tn, 1, W), np.uint8)
    tok[0, 0, 0], cost[0, 0, 0] = START, 0.0
    for t, (t0, t1, c0, c1, p0, p1) in enumerate([(5, 6, 1.0, 1.1, 0, 0), (END, 7, 2.0, 2.1, 0, 1), (END, 8, 2.4, 2.6, 1, 1),
                                                  (9, END, 2.8, 4.0, 1, 1), (END, 3, 3.0, 3.5, 0, 0), (4, 4, 4.0, 4.1, 1, 1)], 1):
        tok[t, 0], cost[t, 0], par[t, 0] = (t0, t1), (c0, c1), (p0, p1)
    end[2, 0, 0] = end[3, 0, 0] = end[4, 0, 1] = end[5, 0, 0] = 1
    return tok, cost, par, end


def test_replay_hypotheses_length_penalty():
    from showtell_amd.beam import replay_hypotheses
    rec = _hand_records()
    A, B, C, D = [1, 5, END], [1, 6, 7, END], [1, 6, 7, 8, END], [1, 6, 7, 8, 9, END]
    c24 = float(np.float32(2.4))
    plain = replay_hypotheses(*rec, 4)
    assert plain == [[(A, 2.0), (B, c24), (D, 3.0), (C, 4.0)]]
    assert replay_hypotheses(*rec, 4, length_penalty=0.0) == plain == replay_hypotheses(*rec, 4, None, 0)
    # cost / n: A 2 / 2 = 1, B 2.4 / 3 = 0.8, C 4 / 4 = 1, D 3 / 5 = 0.6 -> D, B, then the tie A, C in harvest order (stable);
    # the raw cost is returned
    assert replay_hypotheses(*rec, 4, length_penalty=1.0) == [[(D, 3.0), (B, c24), (A, 2.0), (C, 4.0)]]
    assert replay_hypotheses(*rec, 1, length_penalty=1.0) == [[(D, 3.0)]]
    # a = 0.5: A 2 / sqrt 2 = 1.414, B 2.4 / sqrt 3 = 1.386, C 4 / 2 = 2, D 3 / sqrt 5 = 1.342
    assert replay_hypotheses(*rec, 3, length_penalty=0.5) == [[(D, 3.0), (B, c24), (A, 2.0)]]
    # a < 0 favours short captions even more than the raw cost does
    assert [s for s, _ in replay_hypotheses(*rec, 4, length_penalty=-1.0)[0]] == [A, B, D, C]


# ---- argument validation (before any device work, so it needs no GPU) ---------------------------------------------------

def _decoders():
    from showtell_amd.rnn import RNN
    from showtell_amd.rnn_attn import RNN_Attn
    return [RNN(16, 16, 50, 1), RNN_Attn(16, 24, 8, 16, 50, 1)], [torch.zeros(2, 16), torch.zeros(2, 24, 9)]


def test_limits_are_rejected_before_any_device_work():
    from showtell_amd.beam import BeamConstraints, beam_search_host, beam_search_records
    for m, feat in zip(*_decoders()):
        for bad in (dict(no_repeat_ngram_size=17), dict(suppress_tokens=list(range(49)) + list(range(16))), dict(suppress_tokens=[50]),
                    dict(suppress_tokens=[-1]), dict(min_length=-1), dict(no_repeat_ngram_size=1, max_length=64), dict(min_length=1.5),
                    dict(length_penalty=float("nan"))):
            with pytest.raises(ValueError):
                m.beam_search(feat, 4, 1, **bad)
    plain = _decoders()[0][0]
    for fn in (beam_search_records, beam_search_host):
        with pytest.raises(ValueError):
            fn(plain, torch.zeros(2, 16), 4, no_repeat_ngram_size=17)
    with pytest.raises(ValueError):
        BeamConstraints(600000, 20, min_length=1)                         # the ban bitmap holds 524288 entries
    assert not BeamConstraints(600000, 20).active                         # ... which only the constrained path needs
    bc = BeamConstraints(50, 63, 70, 16, list(range(50)) + [0] * 14, 1.0)  # every limit reached; min_length >= max_length is legal
    assert bc.active and bc.keep_paths and (bc.min_length, bc.ngram, len(bc.suppress)) == (70, 16, 64)
    assert BeamConstraints(50, 20, suppress_tokens=[]).active and not BeamConstraints(50, 64, min_length=2).keep_paths


def test_python_limits_are_the_headers():
    import os
    import re
    from showtell_amd import beam
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "showtell_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (ST_BEAM_MAX_[A-Z]+) (\d+)", txt)}
    assert defs == {k: getattr(beam, k) for k in ("ST_BEAM_MAX_NGRAM", "ST_BEAM_MAX_SUPPRESS", "ST_BEAM_MAX_HIST", "ST_BEAM_MAX_VOCAB")}
