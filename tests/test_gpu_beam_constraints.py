"""Constrained beam search on the GPU (min_length, no_repeat_ngram_size, suppress_tokens, length_penalty): the ban kernel
against torch, the no-op identity, the searches' records walked by the float64 oracle, and the loud failures.

The walk is the method of test_gpu_beam_bench_shape.py at small shapes (tests/_beam_oracle.check_records): the oracle
is teacher-forced on the GPU's own records and for every iteration, image and slot checks, exactly, the bookkeeping, that no
recorded token is banned for its parent (ban sets from the plain-Python rule), that nothing is harvested before min_length and
that the paths the search kept are the paths along `par`; and within a bound the step cost against the oracle's UNMASKED -log p
(B: a kernel that renormalised over the unbanned set would move it by -log(1 - banned mass)) and the selection over the oracle's
unbanned candidates (C: chosen ones at most SEL above the W-th, every unbanned one more than SEL below it chosen -- the second
half is what catches over-banning).  B and C leave out no live slot (asserted).

Bounds.  None comes from the kernels: NLL_ABS is 4 x the floor of the case's decoder, the largest |d log p| over the
constraint sets between the same restatement in fp32 and in float64 arithmetic (bf16 storage for the bf16 cases), teacher-forced
on the float64 oracle's own constrained free run; SEL = 2 NLL_ABS (two candidates).  `python -m tests.test_gpu_beam_constraints`
prints the floors on the CPU.  One floor per decoder case, not per constraint set: the fp32 floors of a case's sets lie within 3x of
each other, but a bf16 floor is decided by which few stored values happen to round differently in fp32 and float64 arithmetic on
that run's tokens (5e-7 to 3e-3 nats over the sets of one decoder), and the GPU's own records are other tokens again, so a set's
own floor says little about the error to expect on it.  The largest still lies far below the 0.05 nats by which a kernel that
renormalised over the unbanned set would move the step cost on these inputs (test_beam_constraints_inputs.py).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _beam_constraints_cases as K
from tests._beam_constraints_cases import END, START, T
from tests._beam_oracle import StepOracle, check_records

pytestmark = pytest.mark.gpu

# (kind, cell, dtype name, W, B, V) -> floor (see above); the walk's bound is 4 x
CASES = {
    "plain-gru-fp32": ("plain", "gru", "fp32", 4, 24, 600),
    "plain-lstm-fp32": ("plain", "lstm", "fp32", 4, 24, 600),
    "plain-gru-w8-fp32": ("plain", "gru", "fp32", 8, 9, 2056),
    "attn-gru-fp32": ("attn", "gru", "fp32", 5, 13, 600),
    "attn-lstm-fp32": ("attn", "lstm", "fp32", 5, 13, 600),
    "plain-gru-bf16": ("plain", "gru", "bf16", 4, 24, 600),
    "attn-lstm-bf16": ("attn", "lstm", "bf16", 5, 13, 600),
}
FLOOR = {                                 # the floor of each constraint set; after "|" the GPU's worst |d nll| over the sets
    "plain-gru-fp32": 1.87e-06,           # g1 1.6e-06 g2 1.1e-06 g3 8.6e-07 min6 1.3e-06 sup5 1.9e-06 all 1.8e-06 g1s 1.3e-06 g2s 1.1e-06 | 4.24e-07
    "plain-lstm-fp32": 7.60e-07,          # g1 7.6e-07 g2 5.5e-07 g3 5.1e-07 min6 5.5e-07 sup5 4.2e-07 all 4.4e-07 g1s 7.5e-07 g2s 5.1e-07 | 2.60e-07
    "plain-gru-w8-fp32": 2.08e-06,        # g1 1.1e-06 g2 1.1e-06 g3 9.2e-07 min6 1.9e-06 sup5 2.0e-06 all 2.1e-06 g1s 1.3e-06 g2s 1.0e-06 | 9.42e-07
    "attn-gru-fp32": 2.49e-06,            # g1 2.3e-06 g2 2.4e-06 g3 2.4e-06 min6 2.4e-06 sup5 2.5e-06 all 2.3e-06 g1s 2.4e-06 g2s 2.5e-06 | 1.24e-06
    "attn-lstm-fp32": 8.49e-07,           # g1 5.4e-07 g2 4.6e-07 g3 6.0e-07 min6 5.3e-07 sup5 7.2e-07 all 8.0e-07 g1s 8.5e-07 g2s 8.1e-07 | 4.86e-07
    "plain-gru-bf16": 3.34e-03,           # g1 3.3e-03 g2 5.0e-07 g3 1.3e-03 min6 4.7e-06 sup5 1.2e-03 all 5.6e-04 g1s 3.2e-03 g2s 1.4e-03 | 4.38e-03
    "attn-lstm-bf16": 1.95e-03,           # g1 1.6e-03 g2 2.6e-04 g3 3.7e-04 min6 7.2e-04 sup5 1.9e-03 all 1.1e-03 g1s 1.3e-03 g2s 1.6e-03 | 1.94e-03
}
# the constraint sets on which a decoder's hypotheses are ranked with a length penalty: the combined set, and the set on which
# test_beam_constraints_inputs.py asserts that length_penalty = 1 changes the first hypothesis of a quarter of the images
LP_SETS = {"plain-gru": ("all",), "plain-lstm": ("all", "min6"), "plain-gru-w8": ("all",), "attn-gru": ("all",), "attn-lstm": ("all",)}
_DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
_MODELS = {}


def _model(kind, cell, dtype, vocab, cname="all"):
    key = (kind, cell, dtype, vocab, cname)
    if key not in _MODELS:
        params = {k: v.clone() for k, v in K.decoder_params(kind, cell, vocab, cname).items()}
        if kind == "plain":
            from tests.test_gpu_decoder import _make
            _MODELS[key] = _make(cell, params, _DT[dtype]).eval()
        else:
            from tests.test_gpu_attention_beam import _make
            _MODELS[key] = _make(cell, params, _DT[dtype])
    return _MODELS[key]


def _search(kind, m, feat, W, nh=1, records=True, **kw):
    """(hypotheses, records) of either decoder family"""
    from showtell_amd.beam import beam_search, beam_search_records
    if kind == "attn":
        return m.beam_search(feat, W, nh, T, START, END, return_records=True, **kw)
    lp = kw.pop("length_penalty", 0.0)
    rec = beam_search_records(m, feat, W, T, START, END, **kw) if records else None
    return beam_search(m, feat, W, nh, T, START, END, length_penalty=lp, **kw), rec


def _kw(cons):
    return dict(min_length=cons[0], no_repeat_ngram_size=cons[1], suppress_tokens=cons[2])


# ====================================================================================================================
# 1. st_beam_ban_topk against torch
# ====================================================================================================================

def _ban_topk(x, ldl, V, k, hist, hist_len, g, sup, ban_end):
    from showtell_amd._lib import check, lib
    from showtell_amd.rnn import _cp, _stream
    n = x.shape[0]
    p = torch.full((n, k), -1.0, device="cuda")
    i = torch.full((n, k), -1, device="cuda", dtype=torch.long)
    check(lib().st_beam_ban_topk(_cp(x), ldl, n, V, k, _cp(hist), hist.shape[1] if hist is not None else 0, hist_len, g, _cp(sup),
                                 0 if sup is None else sup.numel(), END, int(ban_end), _cp(p), _cp(i), _stream()), "st_beam_ban_topk")
    return p, i


@pytest.mark.parametrize("V,ldl", [(5003, 5008), (2048, 2048), (2047, 2048), (37, 40), (10243, 10248)])
@pytest.mark.parametrize("k", [1, 5, 8, 12])
def test_ban_topk_kernels_against_torch(k, V, ldl):
    """The threshold form (k <= 8, k * 256 <= V; V = 10243 streams the row instead of keeping it in registers), its first row
    length, the general form and a row shorter than the block, for ngram 0..3 and paths of 1, 2, 7 and 26 tokens with planted
    repeats, <end> banned and not.  Rows as in test_softmax_topk_kernels_against_torch: many exact ties; row 5 constant (more
    than 256 candidates: the serial fallback, with bans); the 64 suppressed ids hold 0, V - 1 and the 12 largest entries of row 7
    (every top-k entry banned) -- at V = 37 they leave 7 entries, fewer than k = 8 or 12: the tail is (p = 0, id = 0).
    Indices are those of torch.sort(stable) on the negated row with banned entries at -inf, exact; probabilities those of the
    UNMASKED softmax at st_softmax_topk's tolerance; with an empty ban set both outputs are st_softmax_topk's bits."""
    from showtell_amd._lib import check, lib
    from showtell_amd.rnn import _cp, _stream
    torch.manual_seed(3)
    n = 37
    x = torch.randn(n, ldl, device="cuda")
    x[:, ::7] = x[:, 3:4]
    x[5, :V] = 0.25
    row = x[:, :V]
    soft = torch.softmax(row, 1)
    top = torch.sort(-row, dim=1, stable=True).indices.cpu()
    g_ = torch.Generator().manual_seed(4)
    if V == 37:
        ids = torch.cat([torch.tensor([0, V - 1]), torch.arange(1, 29)])          # 30 distinct ids: 7 entries stay
        ids = torch.cat([ids, ids, ids])[:64]
    else:
        ids = torch.cat([torch.tensor([0, V - 1]), top[7, :12], torch.randint(0, V, (50,), generator=g_)])
    assert ids.numel() == 64
    # paths over each row's own four largest entries: repeats of every size are common and the bans hit the top of the row
    pick = torch.randint(0, 4, (n, 26), generator=g_)
    hist_cpu = torch.gather(top[:, :4], 1, pick).to(torch.int32)
    hist_cpu[:, 0] = START
    hist_cpu[3, 1:] = hist_cpu[3, 1:2]                                            # one path of a single repeated word
    hist_cpu[8:12, 0] = top[8:12, 0].to(torch.int32)                              # s_0 counts: here it is the row's largest entry
    hist = hist_cpu.cuda()
    p0 = torch.empty(n, k, device="cuda"); i0 = torch.empty(n, k, device="cuda", dtype=torch.long)
    check(lib().st_softmax_topk(_cp(x), ldl, n, V, k, _cp(p0), _cp(i0), 0, _stream()), "st_softmax_topk")
    p, i = _ban_topk(x, ldl, V, k, None, 1, 0, None, False)
    assert torch.equal(i, i0) and torch.equal(p.view(torch.int32), p0.view(torch.int32)), "empty ban set: not st_softmax_topk's bits"
    p, i = _ban_topk(x, ldl, V, k, hist, 26, 0, ids[:0].cuda(), False)
    assert torch.equal(i, i0) and torch.equal(p.view(torch.int32), p0.view(torch.int32)), "empty ban set: not st_softmax_topk's bits"
    biting = 0
    for g in (0, 1, 2, 3):
        for hist_len in (1, 2, 7, 26):
            for ban_end in (False, True):
                for sup in (None, ids):
                    cons = (hist_len if ban_end else 0, g, None if sup is None else sup.tolist())
                    ban = torch.from_numpy(K.ban_mask(hist_cpu[:, None, :hist_len].numpy(), V, cons)).cuda()
                    p, i = _ban_topk(x, ldl, V, k, hist if g else None, hist_len, g, None if sup is None else sup.cuda(), ban_end)
                    order = torch.sort(-row.masked_fill(ban, -float("inf")), dim=1, stable=True).indices[:, :k]
                    have = ((~ban).sum(1, keepdim=True) > torch.arange(k, device="cuda")[None, :])      # successor j exists
                    tag = (g, hist_len, ban_end, sup is not None)
                    assert torch.equal(i, torch.where(have, order, 0)), tag
                    ref = torch.where(have, torch.gather(soft, 1, order), 0.0)
                    assert torch.equal(p[~have], ref[~have]), tag
                    assert torch.allclose(p, ref, rtol=2e-6, atol=1e-9), tag
                    biting += int((i != i0).any())
                    if sup is not None and V == 37 and k >= 8:
                        assert not have[:, 7:].any()                          # fewer than k unbanned entries: the tail is tested
    # of the 64 settings the 32 with the suppress list change the result (row 7 loses its largest entries), and so do the 6 with
    # g = 1 and a path of at least two tokens (every path holds one of its row's four largest entries)
    assert biting >= 38


def test_ban_topk_at_the_largest_vocabulary():
    """V = 524288: the ban bitmap fills its 64 KB of LDS (the kernels ask for more dynamic LDS than the default allows); both
    kernel forms, bans at the first and the last entry and at the top of the row; one entry more is rejected."""
    from showtell_amd._lib import ShowTellHipError
    V = 524288
    g_ = torch.Generator().manual_seed(8)
    x = torch.randn(3, V + 8, generator=g_).cuda()
    x[:, 0] = 9.0; x[:, V - 1] = 8.0                                              # the two largest entries: the row's ends
    row = x[:, :V]
    top = torch.sort(-row, dim=1, stable=True).indices
    sup = torch.cat([torch.tensor([0, V - 1]), top[1, 2:5].cpu(), torch.tensor([V - 33, 31, 32])]).cuda()
    hist = torch.stack([top[:, 3], top[:, 2], top[:, 3]], 1).to(torch.int32).contiguous()   # g = 2: the word after top[3] is banned
    ban = torch.zeros(3, V, dtype=torch.bool, device="cuda")
    ban[:, sup] = True
    ban[torch.arange(3), top[:, 2]] = True
    # float64 reference; a thread sums 2048 exponentials one after the other in fp32 and the block adds 256 partial sums in a tree:
    # (2048 + 8) roundings of 2^-24 at worst, plus a few for exp and the division
    soft, rtol = torch.softmax(row.double(), 1), 2060 * 2.0 ** -24
    for k in (5, 12):                                                             # threshold form (streaming), general form
        p, i = _ban_topk(x, V + 8, V, k, hist, 3, 2, sup, False)
        order = torch.sort(-row.masked_fill(ban, -float("inf")), dim=1, stable=True).indices[:, :k]
        assert torch.equal(i, order) and not ban.gather(1, i).any()
        assert torch.allclose(p.double(), torch.gather(soft, 1, order), rtol=rtol, atol=0.0)
        assert int(i[0, 0]) == int(top[0, 3]) or int(i[0, 0]) == int(top[0, 4])   # entries 0, V - 1 and top[2] are gone
    with pytest.raises(ShowTellHipError):
        _ban_topk(x, V + 8, V + 1, 5, hist, 3, 2, sup, False)


# ====================================================================================================================
# 2. no-op identity
# ====================================================================================================================

@pytest.mark.parametrize("name", ["plain-gru-fp32", "plain-gru-bf16", "attn-lstm-fp32", "attn-lstm-bf16"])
def test_defaults_and_an_empty_ban_set_give_the_unconstrained_records(name):
    """Every constraint at its default runs st_softmax_topk and st_beam_select without paths (st_attn_beam_search without options);
    suppress_tokens=[] is a constrained search with nothing to ban: st_softmax_topk again, and st_beam_select with the paths kept
    (st_attn_beam_search with keep_paths).  Array for array the same."""
    from showtell_amd.beam import beam_search_records
    kind, cell, dtype, W, B, vocab = CASES[name]
    m, feat = _model(kind, cell, dtype, vocab), K.features(kind, B).cuda()
    if kind == "plain":
        base = beam_search_records(m, feat, W, T, START, END)
        dflt = beam_search_records(m, feat, W, T, START, END, min_length=0, no_repeat_ngram_size=0, suppress_tokens=None)
        hyp_b = m.beam_search(feat, W, 3, T, START, END)
        hyp_d = m.beam_search(feat, W, 3, T, START, END, min_length=0, no_repeat_ngram_size=0, suppress_tokens=None, length_penalty=0.0)
        hyp_e, empty = _search(kind, m, feat, W, 3, suppress_tokens=[])
    else:
        hyp_b, base = m.beam_search(feat, W, 3, T, START, END, return_alphas=True, return_records=True)
        hyp_d, dflt = m.beam_search(feat, W, 3, T, START, END, return_alphas=True, return_records=True, min_length=0,
                                    no_repeat_ngram_size=0, suppress_tokens=None, length_penalty=0.0)
        hyp_e, empty = m.beam_search(feat, W, 3, T, START, END, return_alphas=True, return_records=True, suppress_tokens=[])
    assert "hist" not in base and "hist" not in dflt
    live = int(np.isfinite(base["cost"]).sum())
    assert live > T * B * W // 4                                      # the searches run: most slots are filled
    assert set(empty) == set(base) | {"hist"}
    for key in base:
        assert np.array_equal(base[key], dflt[key]), key
        assert base[key].dtype == empty[key].dtype and np.array_equal(base[key].view(np.uint8), empty[key].view(np.uint8)), key
    assert repr(hyp_b) == repr(hyp_d) == repr(hyp_e)
    assert empty["hist"].shape == (B, W, T + 1) and empty["hist"].dtype == np.int32
    assert np.array_equal(empty["hist"].astype(np.int64), K.slot_paths(empty["tok"], empty["par"], T))


# ====================================================================================================================
# 3. the record walk
# ====================================================================================================================

@pytest.mark.parametrize("cname", list(K.CONSTRAINTS))
@pytest.mark.parametrize("name", list(CASES))
def test_constrained_records_follow_the_oracle(name, cname):
    kind, cell, dtype, W, B, vocab = CASES[name]
    cons = K.CONSTRAINTS[cname]
    m, feat = _model(kind, cell, dtype, vocab, cname), K.features(kind, B)
    hyps, rec = _search(kind, m, feat.cuda(), W, 1, **_kw(cons))
    orc = StepOracle(kind, cell, K.decoder_params(kind, cell, vocab, cname), feat, W, storage=dtype == "bf16")
    assert rec["hist"].shape == (B, W, T + 1)                         # both decoder families hand out the paths they kept
    check_records(rec, orc, 4 * FLOOR[name], f"{name} {cname}", cons, hist=rec["hist"])
    for hyp in hyps:                                                  # well formed, and constrained
        for h in hyp:
            seq = h[0]
            assert seq[0] == START and seq[-1] == END and len(seq) - 2 >= cons[0]
            assert not set(seq[1:]) & set(cons[2] or ())
            g = cons[1]
            if g:
                grams = [tuple(seq[i:i + g]) for i in range(len(seq) - g + 1)]
                assert len(grams) == len(set(grams)), (seq, "an n-gram repeats")


@pytest.mark.parametrize("name,cname", [(n, c) for n in CASES for c in LP_SETS[n.rsplit("-", 1)[0]]])
def test_length_penalty_ranks_the_replayed_hypotheses(name, cname):
    """beam_search(length_penalty=a) is replay_hypotheses(records, length_penalty=a) and the order is that of cost / n**a (float64),
    ties stable, the raw cost returned"""
    from showtell_amd.beam import replay_hypotheses
    kind, cell, dtype, W, B, vocab = CASES[name]
    cons = K.CONSTRAINTS[cname]
    m, feat = _model(kind, cell, dtype, vocab, cname), K.features(kind, B).cuda()
    _, rec = _search(kind, m, feat, W, 1, **_kw(cons))
    raw = replay_hypotheses(rec["tok"], rec["cost"], rec["par"], rec["end"], W * T)
    for a in (0.0, 0.7, 1.0):
        for nh in (1, 3):
            got, _ = _search(kind, m, feat, W, nh, records=False, length_penalty=a, **_kw(cons))
            want = replay_hypotheses(rec["tok"], rec["cost"], rec["par"], rec["end"], nh, length_penalty=a)
            assert [[(s, c) for s, c, *_ in h] for h in got] == [[(s, c) for s, c, *_ in h] for h in want]
            for b, hyp in enumerate(got):
                pool = [(s, c) for s, c, *_ in raw[b]]
                rank = sorted(pool, key=lambda e: float(np.float32(e[1])) / float(len(e[0]) - 1) ** a)[:nh]
                assert [(s, c) for s, c, *_ in hyp] == rank, (a, nh, b)


@pytest.mark.parametrize("cname", list(K.CONSTRAINTS))
@pytest.mark.parametrize("bw,nh,dtype", [(4, 3, "fp32"), (8, 2, "fp32"), (4, 1, "bf16"), (9, 1, "fp32")])
def test_constrained_device_selection_equals_host_bookkeeping(bw, nh, dtype, cname):
    """test_beam_search_device_selection_equals_host_bookkeeping with the constraints on: the device loop (st_beam_ban_topk +
    st_beam_select with its paths) and beam_search_host (paths kept beside its Node table, successors from st_beam_ban_topk) give the same
    sequences; bw = 9 exceeds W * k <= 64 and takes the host path by itself, where the hypotheses must still obey the constraints."""
    from showtell_amd.beam import beam_search, beam_search_host
    cons = K.CONSTRAINTS[cname]
    m, feat = _model("plain", "gru", dtype, 600, cname), K.features("plain", 24).cuda()
    for a in (0.0, 1.0):
        dev = beam_search(m, feat, bw, nh, T, START, END, length_penalty=a, **_kw(cons))
        host = beam_search_host(m, feat, bw, nh, T, START, END, length_penalty=a, **_kw(cons))
        assert len(dev) == len(host) == 24
        for d_, h_ in zip(dev, host):
            assert [s for s, _ in d_] == [s for s, _ in h_]
            for (s, cd), (_, ch) in zip(d_, h_):
                assert abs(cd - ch) <= 1e-5 * max(1.0, abs(ch))
                assert len(s) - 2 >= cons[0] and not set(s[1:]) & set(cons[2] or ())
                if cons[1]:
                    grams = [tuple(s[i:i + cons[1]]) for i in range(len(s) - cons[1] + 1)]
                    assert len(grams) == len(set(grams))


@pytest.mark.parametrize("cname", list(K.CONSTRAINTS))
def test_host_fallback_at_w9_against_the_oracle_free_run(cname):
    """W = 9 (W * k > 64: beam_search is beam_search_host, which keeps no records to walk) against the float64 oracle's own
    constrained search of the same inputs.  A candidate's cumulative cost is off by at most T x NLL_ABS (the W = 4 case's bound per
    step), so two candidates can change places only when they lie within MARGIN = 2 T NLL_ABS.  On an image whose oracle run keeps
    every first-left-out candidate more than MARGIN above the last one taken, and whose two best hypotheses are further apart than
    that, both searches make the same choices: the first hypothesis must be the oracle's, token for token, at its cost.  That is
    the case for most images (asserted).  A search that banned too much or too little would leave the oracle's path."""
    from showtell_amd.beam import beam_search, replay_hypotheses
    W, B = 9, 24
    cons = K.CONSTRAINTS[cname]
    nll_abs = 4 * FLOOR["plain-gru-fp32"]
    margin = 2 * T * nll_abs
    m, feat = _model("plain", "gru", "fp32", 600, cname), K.features("plain", B)
    got = beam_search(m, feat.cuda(), W, 2, T, START, END, **_kw(cons))
    orc = StepOracle("plain", "gru", K.decoder_params("plain", "gru", 600, cname), feat, W, storage=False)
    rec = K.free_run(orc, cons)
    want = replay_hypotheses(rec["tok"], rec["cost"], rec["par"], rec["end"], 2)
    safe = 0
    for b in range(B):
        if rec["gap"][:, b].min() <= margin or not want[b] or (len(want[b]) == 2 and want[b][1][1] - want[b][0][1] <= margin):
            continue
        safe += 1
        assert got[b] and got[b][0][0] == want[b][0][0], (cname, b)
        # T steps of NLL_ABS, and T float32 roundings of the cumulative cost
        assert abs(got[b][0][1] - want[b][0][1]) <= T * nll_abs + T * float(np.spacing(np.float32(want[b][0][1]))), (cname, b)
    print(f"MEASURE host fallback W=9 {cname}: {safe} of {B} images compared")
    assert safe >= B // 2


# ====================================================================================================================
# 4. loud failures
# ====================================================================================================================

@pytest.mark.parametrize("kind,cell", [("plain", "gru"), ("attn", "lstm")])
def test_limits_are_rejected_loudly(kind, cell):
    from showtell_amd._lib import ShowTellHipError
    m, feat = _model(kind, cell, "fp32", 600), K.features(kind, 3).cuda()
    for bad in (dict(no_repeat_ngram_size=17), dict(suppress_tokens=list(range(65))), dict(suppress_tokens=[600]),
                dict(suppress_tokens=[-1]), dict(min_length=-1), dict(no_repeat_ngram_size=2, max_length=64)):
        with pytest.raises(ValueError):
            m.beam_search(feat, 4, 1, **bad)
    assert m.beam_search(feat, 4, 1, max_length=5, min_length=5) == [[], [], []]      # legal: nothing can end in time
    m.beam_search(feat, 4, 1, max_length=64, min_length=1)                            # no paths needed without n-gram blocking
    # the C entry points check for themselves
    x = torch.randn(2, 40, device="cuda")
    hist = torch.ones(2, 8, device="cuda", dtype=torch.int32)
    for args in ((hist, 2, 17, None), (None, 2, 2, None), (hist, 9, 2, None), (hist, 2, 0, torch.zeros(65, dtype=torch.long, device="cuda"))):
        with pytest.raises(ShowTellHipError):
            _ban_topk(x, 40, 37, 4, args[0], args[1], args[2], args[3], False)
    if kind == "attn":
        from showtell_amd._lib import check, lib
        from showtell_amd.rnn import _cp, _stream
        prm, keep, featc, B, P = m._decode_inputs(feat)
        from showtell_amd._lib import BeamOpts

        def opts(ngram=0, n_suppress=0, keep_paths=1):
            return C.byref(BeamOpts(0, ngram, _cp(tok), n_suppress, keep_paths, 1, 0.0))

        def planned(mlen, o):
            return lib().st_attn_beam_workspace_bytes(C.byref(prm), B, 4, mlen, o, None)

        tok = torch.empty(65, B, 4, device="cuda", dtype=torch.long); cost = torch.empty(65, B, 4, device="cuda")
        nb = planned(64, opts(keep_paths=0))
        assert nb == planned(64, None) == planned(14, None) > 0                       # max_length = 64: no path buffers
        assert planned(14, opts()) > nb and planned(64, opts()) == 0                  # ... and none can be asked for
        ws = torch.empty(nb, device="cuda", dtype=torch.uint8)
        par = torch.empty(65, B, 4, device="cuda", dtype=torch.int32); end = torch.empty(64, B, 4, device="cuda", dtype=torch.uint8)
        for mlen, g, ns, kp in ((64, 2, 0, 0), (14, 17, 0, 1), (14, 0, 65, 1), (14, -1, 0, 1), (14, 2, 0, 0), (64, 0, 0, 1)):
            with pytest.raises(ShowTellHipError):
                check(lib().st_attn_beam_search(C.byref(prm), _cp(featc), B, 4, mlen, START, END, _cp(ws), nb, _cp(tok), _cp(cost), _cp(par),
                                                _cp(end), None, opts(g, ns, kp), _stream()), "st_attn_beam_search")


if __name__ == "__main__":
    torch.set_num_threads(8)
    for name_, (kind_, cell_, dtype_, W_, B_, vocab_) in CASES.items():
        fl = {c: K.floor(kind_, cell_, dtype_ == "bf16", W_, B_, vocab_, c) for c in K.CONSTRAINTS}
        print(f'    "{name_}": {max(fl.values()):.2e},      # ' + " ".join(f"{c} {v:.1e}" for c, v in fl.items()), flush=True)
