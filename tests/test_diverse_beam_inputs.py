"""Diverse (group) beam search without a GPU: the inputs of test_gpu_diverse_beam.py have the power to fail a wrong kernel (asserted
from the float64 oracle's own diverse search), the sufficiency of the k-lists, the numpy float32 replica against the plain-Python
rule, seeded faults of the rule against the group walk, the helpers (group_records, distinct_ngrams) and argument validation.

Measured on the float64 oracle (MEASURE lines), decoders of _diverse_beam_cases.INPUTS, unconstrained, cases 1 .. 6 at lam 0.5 / 2.0:
filled slots decided by the penalty 196 of 1242 / 151 of 1004, 289 of 1180 / 422 of 1200, 222 of 888 / 346 of 890, 200 of 956 / 288
of 924, 212 of 813 / 429 of 933, 265 of 799 / 287 of 508; group-steps in which a membership test instead of the count changes the
chosen set at lam = 0.5: 42 / 45 / 75 / 56 / 38 / 186 (at lam = 2.0 almost none: that fault is judged at 0.5); (image, group) pairs
that finish while another group of the image lives 16 / 16, 7 / 6, 6 / 9, 10 / 14, 11 / 3, 20 / 51; distinct-2 of the best-per-group
captions higher at lam = 0.5 than at 0 on 14 of 24, 23 of 24, 9 of 9, 13 of 13, 13 of 13, 8 of 9 images, lower on none; smallest key
gap at a cut 1.1e-4 nats (case 3), above the walk's selection tolerance on fp32 records, 8 x 2.1e-6."""
import numpy as np
import pytest
import torch

from tests import _beam_constraints_cases as K
from tests import _diverse_beam_cases as D
from tests._beam_constraints_cases import END, START, T
from tests._beam_oracle import as_recorded, check_records

NLL_ABS = 4 * 2.5e-6          # the walk's bound on float64 records: 4 x the largest fp32 floor of test_gpu_diverse_beam
MAIN = ("plain-gru", "plain-lstm", "attn-gru", "attn-lstm")     # cases 1, 2, 4 and 5
_RUNS = {}


def _run(name, lam, cname=None, **kw):
    key = (name, lam, cname, tuple(sorted(kw.items())))
    if key not in _RUNS:
        _RUNS[key] = D.free_run(D.oracle(name), D.DECODERS[name][3], lam, K.CONSTRAINTS[cname] if cname else D.NONE, **kw)
    return _RUNS[key]


# ---- the inputs -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", MAIN)
def test_without_penalty_every_group_repeats_group_0(name):
    from showtell_amd.beam import group_records
    G = D.DECODERS[name][3]
    rec = _run(name, 0.0)
    g0 = group_records(rec, 0, G)
    assert np.isfinite(g0["cost"]).sum() > T * rec["tok"].shape[1]            # the search runs
    for g in range(1, G):
        r = group_records(rec, g, G)
        for key in ("tok", "cost", "par", "end"):
            assert np.array_equal(r[key], g0[key]), (g, key)


@pytest.mark.parametrize("name", list(D.DECODERS))
def test_the_penalty_decides_and_the_count_matters(name):
    G = D.DECODERS[name][3]
    for lam in D.LAMBDAS:
        rec = _run(name, lam)
        filled = int((rec["par"][1:] >= 0).sum())
        decided = int(rec["decided"].sum())
        diff = int(rec["member_diff"].sum())
        gap = float(rec["gap"].min())
        print(f"MEASURE {name} lam={lam}: decided by the penalty {decided} of {filled} filled slots; count != membership in {diff} "
              f"group-steps; smallest key gap at the cut {gap:.2e}")
        assert filled >= 500 and decided >= 0.15 * filled
        if lam == 0.5:
            assert diff >= 20
        check_records(as_recorded(rec), D.oracle(name), NLL_ABS, f"{name} lam={lam} float64 free run", D.NONE, G, lam)


def _early(rec):
    """(image, group) pairs whose group has no live slot at an iteration at which another group of the image still has one"""
    live = rec["live_g"]                                                           # [T][B][G]
    return int(((~live) & live.any(2, keepdims=True)).any(0).sum())


@pytest.mark.parametrize("name", list(D.DECODERS))
def test_groups_finish_while_others_live(name):
    """the per-group done flags are exercised on every case: at least 5 (image, group) pairs finish while another group of the image
    is still live, counted at lam = 0.5 alone (the penalty at which the seeded faults are judged); lam = 2.0 is reported.  A group
    of W' slots finishes only when all of them end in the same iteration, which is why the decoders' <end> rows are sharpened"""
    n5, n2 = _early(_run(name, 0.5)), _early(_run(name, 2.0))
    print(f"MEASURE {name}: (image, group) pairs finished while another group lives: {n5} at lam = 0.5, {n2} at lam = 2.0")
    assert n5 >= 5 and n2 >= 1


@pytest.mark.parametrize("name", list(D.DECODERS))
def test_the_penalty_makes_the_captions_differ(name):
    """distinct-2 over each image's best-per-group captions at lam = 0.5 against lam = 0 (where every group finds group 0's
    caption): lower on no image, higher on more than half of the images of every case -- on the others the groups still agree on
    their best caption, or (W' = 1 only) nothing ends in time -- and every image has a caption at lam = 0.5 on the four main cases"""
    from showtell_amd.evaluation import distinct_ngrams
    G = D.DECODERS[name][3]
    c0, c5 = D.best_per_group(_run(name, 0.0), G), D.best_per_group(_run(name, 0.5), G)
    d0, d5 = [distinct_ngrams(c, 2) for c in c0], [distinct_ngrams(c, 2) for c in c5]
    higher = sum(a > b for a, b in zip(d5, d0))
    with_caption = sum(bool(c) for c in c5)
    print(f"MEASURE {name}: distinct-2 of the best-per-group captions, mean over images {np.mean(d0):.3f} at lam = 0, {np.mean(d5):.3f} "
          f"at lam = 0.5; higher on {higher} of {len(d0)} images, lower on {sum(a < b for a, b in zip(d5, d0))}; images with a caption "
          f"at lam = 0.5: {with_caption}")
    assert all(a >= b for a, b in zip(d5, d0)) and higher > len(d0) // 2
    assert with_caption == len(c5) or name not in MAIN


@pytest.mark.parametrize("cname", [None, "all"])
@pytest.mark.parametrize("name", list(D.DECODERS))
def test_the_k_lists_suffice(name, cname):
    """k = min(W, V) words per node are enough: the search over ALL words of every node makes the same choices, exactly"""
    for lam in D.LAMBDAS:
        a, b = _run(name, lam, cname), _run(name, lam, cname, all_v=True)
        for key in ("tok", "cost", "par", "end"):
            assert np.array_equal(a[key], b[key]), (lam, key)


def test_the_float32_replica_is_the_rule():
    """hand-built fringes (shared words, empty and ended slots, finished groups, missing successors): the numpy replica against the
    plain-Python rule in float64, wherever the keys of a group lie further apart than float32 rounding"""
    compared = 0
    for W, G, k in ((4, 2, 4), (6, 3, 6), (8, 2, 8), (8, 4, 8), (8, 8, 8), (6, 2, 5)):
        Wg = W // G
        for lam in (0.0, 0.5, 2.0):
            tok, cost, done, p, ids = D.hand_fringes(W, G, k)
            B = tok.shape[0]
            got = D.select_groups_f32(tok, cost, done, p, ids, G, END, lam)
            grp = np.arange(W) // Wg
            for b in range(B):
                occupied = np.isfinite(cost[b])
                live = occupied & (tok[b] != END) & ~done[b].astype(bool)[grp]
                raw = [[float(cost[b, w]) - float(np.log(np.float64(q))) if live[w] and q > 0 else D.INF for q in p[b * W + w][::-1]]
                       for w in range(W)]
                words = [ids[b * W + w][::-1].tolist() for w in range(W)]
                new = D.rule_image(raw, words, W, G, lam)
                keys = [sorted(x for x in D._keys_of_group(raw, words, new, g, Wg, lam) if x < D.INF) for g in range(G)]
                if any(np.diff(ks).min() < 1e-5 for ks in keys if len(ks) > 1):
                    continue
                compared += 1
                assert [e[0] if e else -1 for e in new] == got["par"][b].tolist()
                assert [e[1] if e else 0 for e in new] == got["tok"][b].tolist()
                assert np.allclose([e[2] if e else np.inf for e in new], got["cost"][b], rtol=3e-7, atol=0)
    assert compared >= 300


# ---- seeded faults ----------------------------------------------------------------------------------------------------

FAULTS = {                                                                # name -> (lam, constraint set, free_run arguments)
    "the penalty added into the recorded cost": (0.5, None, dict(penalty_in_cost=True)),
    "the penalty subtracted": (0.5, None, dict(sign=-1.0)),
    "n_v counted over all groups": (0.5, None, dict(scope="all")),
    "n_v counted over the previous fringe": (0.5, None, dict(scope="prev")),
    "membership instead of count": (0.5, None, dict(member=True)),
    "groups above 0 left unseeded": (0.5, None, dict(unseeded=True)),
    "one done flag per image": (0.5, None, dict(done_per_image=True)),
    "a parent taken from another group": (0.5, None, dict(cross_parent=True)),
    "bans applied after the penalty cut": (0.5, "all", dict(after_cut=True)),
}


@pytest.mark.parametrize("fault", list(FAULTS))
@pytest.mark.parametrize("name", MAIN)
def test_seeded_faults_are_caught_by_the_group_walk(name, fault):
    """each fault runs the float64 oracle's own diverse search with the broken rule on the inputs of a GPU case; the walk of its
    records, the checks of test_gpu_diverse_beam.py, must fail, and passes on the unbroken search"""
    lam, cname, kw = FAULTS[fault]
    G = D.DECODERS[name][3]
    cons = K.CONSTRAINTS[cname] if cname else D.NONE
    check_records(as_recorded(_run(name, lam, cname)), D.oracle(name), NLL_ABS, f"{name} unbroken", cons, G, lam)
    with pytest.raises(AssertionError):
        check_records(as_recorded(_run(name, lam, cname, **kw)), D.oracle(name), NLL_ABS, f"{name} {fault}", cons, G, lam)


# ---- helpers ----------------------------------------------------------------------------------------------------------

def test_group_records_slices_and_rebases():
    from showtell_amd.beam import group_records, replay_groups, replay_hypotheses
    rec = _run("attn-gru", 0.5)
    B, W = rec["tok"].shape[1:]
    full = dict(tok=rec["tok"], cost=rec["cost"].astype(np.float32), par=rec["par"], end=rec["end"],
                hist=K.slot_paths(rec["tok"], rec["par"], T, 3).astype(np.int32),
                alpha=np.arange(T * B * W * 2, dtype=np.float32).reshape(T, B * W, 2))
    for g in range(3):
        r = group_records(full, g, 3)
        assert r["tok"].shape == (T + 1, B, 2) and r["end"].shape == (T, B, 2) and r["hist"].shape == (B, 2, T + 1)
        assert r["par"].min() == -1 and r["par"].max() == 1
        assert np.array_equal(r["par"] >= 0, full["par"][:, :, 2 * g:2 * g + 2] >= 0)
        assert np.array_equal(r["alpha"], full["alpha"].reshape(T, B, W, 2)[:, :, 2 * g:2 * g + 2].reshape(T, B * 2, 2))
        assert np.array_equal(r["hist"].astype(np.int64), K.slot_paths(r["tok"], r["par"], T))     # a search of its own
    hyps = replay_groups(full, 3, 2, 0.7)
    assert len(hyps) == B and all(len(h) == 3 for h in hyps)
    for g in range(3):
        r = group_records(full, g, 3)
        want = replay_hypotheses(r["tok"], r["cost"], r["par"], r["end"], 2, r["alpha"], 0.7)
        for b in range(B):
            assert [(s, c) for s, c, _ in hyps[b][g]] == [(s, c) for s, c, _ in want[b]]
            assert all(torch.equal(x[2], y[2]) and x[2].shape == (len(x[0]) - 1, 2) for x, y in zip(hyps[b][g], want[b]))
    assert sum(len(x) for h in hyps for x in h) > B
    with pytest.raises(ValueError):
        group_records(full, 3, 3)
    with pytest.raises(ValueError):
        group_records(full, 0, 4)


def test_distinct_ngrams():
    from showtell_amd.evaluation import distinct_ngrams
    assert distinct_ngrams([[1, 2, 3], [1, 2, 3]], 1) == 0.5 and distinct_ngrams([[1, 2, 3], [1, 2, 3]], 2) == 0.5
    assert distinct_ngrams([[1, 2, 3], [1, 2, 4]], 2) == 0.75 and distinct_ngrams([[1, 2, 3], [4, 5, 6]], 3) == 1.0
    assert distinct_ngrams([[1, 1, 1, 1]], 2) == 1 / 3 and distinct_ngrams([[1], []], 2) == 0.0 and distinct_ngrams([], 1) == 0.0
    with pytest.raises(ValueError):
        distinct_ngrams([[1, 2]], 0)


# ---- argument validation (before any device work, so it needs no GPU) ---------------------------------------------------

def _decoders():
    from showtell_amd.rnn import RNN
    from showtell_amd.rnn_attn import RNN_Attn
    from showtell_amd.rnn_attn_LSTM import RNN_Attn as RNN_Attn_LSTM
    from showtell_amd.rnn_lstm import RNN as RNN_LSTM
    plain, attn = torch.zeros(2, 16), torch.zeros(2, 24, 9)
    return [(RNN(16, 16, 50, 1), plain), (RNN_LSTM(16, 16, 50, 1), plain), (RNN_Attn(16, 24, 8, 16, 50, 1), attn),
            (RNN_Attn_LSTM(16, 24, 8, 16, 50, 1), attn)]


BAD_GROUPS = (dict(beam_width=4, num_beam_groups=0), dict(beam_width=4, num_beam_groups=5), dict(beam_width=4, num_beam_groups=1.5), dict(beam_width=4, num_beam_groups=2.0),
              dict(beam_width=4, num_beam_groups="two"), dict(beam_width=4, num_beam_groups=-2), dict(beam_width=6, num_beam_groups=4),
              dict(beam_width=4, num_beam_groups=2, diversity_penalty=-0.5), dict(beam_width=4, num_beam_groups=2, diversity_penalty=float("nan")),
              dict(beam_width=4, num_beam_groups=1, diversity_penalty=0.5))


def test_group_arguments_are_rejected_before_any_device_work():
    from showtell_amd import beam
    for m, feat in _decoders():
        for bad in BAD_GROUPS:
            with pytest.raises(ValueError):
                m.beam_search(feat, **bad)
    plain, feat = _decoders()[0]
    for bad in BAD_GROUPS:
        for fn in (beam.beam_search, beam.beam_search_records, beam.beam_search_host):
            with pytest.raises(ValueError):
                fn(plain, feat, **bad)
    # diverse search runs on the device only
    with pytest.raises(ValueError, match="on the device only") as e_host:
        beam.beam_search_host(plain, feat, 4, num_beam_groups=2, diversity_penalty=0.5)
    with pytest.raises(ValueError, match="on the device only") as e_off:
        beam.beam_search(plain, feat, 4, on_device=False, num_beam_groups=2)
    with pytest.raises(ValueError, match="on the device only") as e_wide:
        beam.beam_search(plain, feat, 10, num_beam_groups=2)                              # 10 * 10 > 64
    assert str(e_host.value) == str(e_off.value) == str(e_wide.value) == beam.DIVERSE_ON_DEVICE_ONLY
    assert beam.check_groups(8, 50, 8, 2) == (8, 2.0) and beam.check_groups(9, 50, 1, 0.0, on_device=False) == (1, 0.0)
    assert beam.check_groups(12, 5, 3, 0.5) == (3, 0.5)                                   # W * min(W, V) = 60
    assert beam.check_groups(4, 50, np.int64(2), np.float32(0.5)) == (2, 0.5)
