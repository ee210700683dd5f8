"""Diverse (group) beam search on the GPU (num_beam_groups, diversity_penalty): the selection kernel against a numpy float32
replica on hand-built fringes, G = 1 against the recorded outputs of the single-beam kernel it replaced, the searches' records walked group by
group by the float64 oracle, the returned hypotheses against the replayed groups, and the loud failures.

The walk is tests/_beam_oracle.check_records: test_gpu_beam_constraints.py's method per group.  The oracle is
teacher-forced on the GPU's own records and checks, exactly, the bookkeeping of every group (seeding, harvest flags and done per
group, parents inside the group, slots filled, keys ascending, no recorded token banned, hist = the paths along par) and, within a
bound, the step cost against the oracle's unmasked -log p (B: the recorded cost must not contain the penalty) and the selection of
every group over the oracle's candidates keyed with lam * n_v (C).  B and C leave out no live slot (asserted).

Bounds.  None comes from the kernels: NLL_ABS is 4 x the floor of the case, the largest |d log p| over the two penalties and the
two constraint settings between the same restatement in fp32 and in float64 arithmetic (bf16 storage for the bf16 cases),
teacher-forced on the float64 oracle's own diverse search; SEL = 2 NLL_ABS (two candidates).  `python -m tests.test_gpu_diverse_beam`
prints the floors on the CPU.  The penalties are dyadic (0.5 and 2.0), so lam * n_v is exact in every precision, and the smallest key
gap at a cut of the oracle's own runs (1.1e-4 nats over the six decoders, test_diverse_beam_inputs.py prints it) lies above the
largest fp32 SEL of 1.6e-5, so that check C discriminates at every cut of the fp32 cases.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import _beam_constraints_cases as K
from tests import _diverse_beam_cases as D
from tests._beam_constraints_cases import END, START, T
from tests._beam_oracle import check_records

pytestmark = pytest.mark.gpu

# case -> (decoder of _diverse_beam_cases, dtype name)
CASES = {
    "plain-gru-fp32": ("plain-gru", "fp32"),
    "plain-gru-bf16": ("plain-gru", "bf16"),
    "plain-lstm-fp32": ("plain-lstm", "fp32"),
    "plain-gru-w8-fp32": ("plain-gru-w8", "fp32"),
    "attn-gru-fp32": ("attn-gru", "fp32"),
    "attn-lstm-fp32": ("attn-lstm", "fp32"),
    "attn-lstm-bf16": ("attn-lstm", "bf16"),
    "plain-gru-g8-fp32": ("plain-gru-g8", "fp32"),
}
FLOOR = {                                 # the floor of each (lam, constraint setting); after "|" the GPU's worst |d nll| over them
    "plain-gru-fp32": 1.53e-06,       # 0.5/free 1.5e-06 0.5/all 1.5e-06 2.0/free 1.5e-06 2.0/all 1.2e-06 | 4.20e-07
    "plain-gru-bf16": 2.73e-04,       # 0.5/free 3.1e-06 0.5/all 2.7e-04 2.0/free 3.1e-06 2.0/all 2.7e-04 | 9.76e-04
    "plain-lstm-fp32": 7.15e-07,      # 0.5/free 6.3e-07 0.5/all 7.2e-07 2.0/free 6.3e-07 2.0/all 6.4e-07 | 1.85e-07
    "plain-gru-w8-fp32": 2.05e-06,    # 0.5/free 1.7e-06 0.5/all 1.6e-06 2.0/free 2.1e-06 2.0/all 1.6e-06 | 6.63e-07
    "attn-gru-fp32": 2.28e-06,        # 0.5/free 2.3e-06 0.5/all 2.3e-06 2.0/free 2.3e-06 2.0/all 2.3e-06 | 1.12e-06
    "attn-lstm-fp32": 7.51e-07,       # 0.5/free 4.4e-07 0.5/all 5.8e-07 2.0/free 4.6e-07 2.0/all 7.5e-07 | 4.69e-07
    "attn-lstm-bf16": 1.54e-03,       # 0.5/free 1.5e-03 0.5/all 3.3e-05 2.0/free 1.5e-03 2.0/all 3.3e-05 | 2.14e-03
    "plain-gru-g8-fp32": 1.21e-06,    # 0.5/free 1.1e-06 0.5/all 1.2e-06 2.0/free 8.4e-07 2.0/all 1.2e-06 | 5.30e-07
}
SETTINGS = {"free": D.NONE, "all": K.CONSTRAINTS["all"]}
_DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
_MODELS, _RECORDS = {}, {}


def _model(case):
    if case not in _MODELS:
        name, dtype = CASES[case]
        kind, cell = D.DECODERS[name][:2]
        params = {k: v.clone() for k, v in D.decoder_params(name).items()}
        if kind == "plain":
            from tests.test_gpu_decoder import _make
            _MODELS[case] = _make(cell, params, _DT[dtype]).eval()
        else:
            from tests.test_gpu_attention_beam import _make
            _MODELS[case] = _make(cell, params, _DT[dtype])
    return _MODELS[case]


def _kw(cons):
    return dict(min_length=cons[0], no_repeat_ngram_size=cons[1], suppress_tokens=cons[2])


def _search(case, lam, cons, nh=1, alphas=False, **kw):
    """(hypotheses, records) of either decoder family"""
    from showtell_amd.beam import beam_search, beam_search_records
    name, _ = CASES[case]
    kind, _, W, G, B, _ = D.DECODERS[name]
    m, feat = _model(case), K.features(kind, B).cuda()
    kw = dict(num_beam_groups=G, diversity_penalty=lam, **_kw(cons), **kw)
    if kind == "attn":
        return m.beam_search(feat, W, nh, T, START, END, return_alphas=alphas, return_records=True, **kw)
    lp = kw.pop("length_penalty", 0.0)
    return beam_search(m, feat, W, nh, T, START, END, length_penalty=lp, **kw), beam_search_records(m, feat, W, T, START, END, **kw)


def _records(case, lam, setting):
    key = (case, lam, setting)
    if key not in _RECORDS:
        _RECORDS[key] = _search(case, lam, SETTINGS[setting])
    return _RECORDS[key]


# ====================================================================================================================
# (a), (b) st_beam_select on hand-built fringes
# ====================================================================================================================

def _select_groups(tok, cost, done, p, ids, G, lam, hist=None, hist_len=0, k=None):
    """the kernel on numpy inputs; every output poisoned first.  Returns dict as D.select_groups_f32 (done = the updated flags)"""
    from showtell_amd._lib import check, lib
    from showtell_amd.rnn import _cp, _stream
    B, W = tok.shape
    k = p.shape[1] if k is None else k
    dev = "cuda"
    t_tok, t_cost, t_done = torch.from_numpy(tok).to(dev), torch.from_numpy(cost).to(dev), torch.from_numpy(done.copy()).to(dev).view(-1)
    t_p, t_i = torch.from_numpy(p).to(dev), torch.from_numpy(ids).to(dev)
    o_tok = torch.full((B, W), -7, device=dev, dtype=torch.long); o_cost = torch.full((B, W), -7.0, device=dev)
    o_par = torch.full((B, W), -7, device=dev, dtype=torch.int32); o_end = torch.full((B, W), 7, device=dev, dtype=torch.uint8)
    o_g = torch.full((B * W,), -7, device=dev, dtype=torch.int32)
    h_in = h_out = None
    if hist is not None:
        h_in = torch.from_numpy(hist).to(dev)
        h_out = torch.full_like(h_in, -7)
    check(lib().st_beam_select(_cp(t_tok), _cp(t_cost), _cp(t_done), _cp(t_p), _cp(t_i), B, W, G, k, END, float(lam), _cp(o_tok),
                               _cp(o_cost), _cp(o_par), _cp(o_end), _cp(o_g), _cp(h_in), _cp(h_out),
                               hist.shape[1] if hist is not None else 0, hist_len, _stream()), "st_beam_select")
    out = dict(tok=o_tok.cpu().numpy(), cost=o_cost.cpu().numpy(), par=o_par.cpu().numpy(), end=o_end.cpu().numpy(),
               gather=o_g.cpu().numpy().reshape(B, W), done=t_done.cpu().numpy().reshape(B, -1))
    if hist is not None:
        out["hist"] = h_out.cpu().numpy()
    return out


def _hist_for(tok, hist_len, ld, seed=3):
    rng = np.random.default_rng(seed)
    h = rng.integers(3, 40, (tok.size, ld)).astype(np.int32)
    h[:, hist_len - 1] = tok.reshape(-1)
    return h


@pytest.mark.parametrize("with_hist", [False, True])
@pytest.mark.parametrize("W,G,k", [(4, 2, 4), (6, 3, 6), (8, 2, 8), (8, 4, 8), (8, 8, 8), (6, 2, 5)])
def test_selection_kernel_against_the_replica(W, G, k, with_hist):
    """every integer output exact, costs within one float32 ulp; the inputs (D.hand_fringes) hold empty and ended slots, finished
    groups, p = 0 entries, words shared by two and three earlier slots and exact key ties made from identical p"""
    tok, cost, done, p, ids = D.hand_fringes(W, G, k)
    B = tok.shape[0]
    hist_len, ld = 5, 9
    hist = _hist_for(tok, hist_len, ld) if with_hist else None
    worst, ties, shared3 = 0.0, 0, 0
    for lam in (0.0, 0.5, 2.0):
        want = D.select_groups_f32(tok, cost, done, p, ids, G, END, lam, hist, hist_len)
        got = _select_groups(tok, cost, done, p, ids, G, lam, hist, hist_len)
        for key in ("tok", "par", "end", "gather", "done"):
            assert np.array_equal(got[key], want[key]), (lam, key)
        fin = np.isfinite(want["cost"])
        assert np.array_equal(np.isfinite(got["cost"]), fin) and (got["cost"][~fin] == np.inf).all()
        ulp = np.abs(got["cost"][fin].astype(np.float64) - want["cost"][fin]) / np.spacing(want["cost"][fin])
        worst = max(worst, float(ulp.max()))
        assert ulp.max() <= 1.0, lam
        if with_hist:
            rows = np.repeat(want["par"].reshape(-1) >= 0, hist_len + 1).reshape(-1, hist_len + 1)
            assert np.array_equal(got["hist"][:, :hist_len + 1], want["hist"][:, :hist_len + 1]), lam
            assert (got["hist"][:, hist_len + 1:] == -7).all() and (got["hist"][:, :hist_len + 1][~rows] == 0).all()
        c = want["cost"].reshape(B, G, W // G)
        ties += int((np.isfinite(c[:, :, :-1]) & (c[:, :, :-1] == c[:, :, 1:])).sum())
        t = want["tok"]
        shared3 += int(((t[:, :, None] == t[:, None, :]) & (want["par"] >= 0)[:, None, :]).sum(2).max() >= 3)
    print(f"MEASURE select_groups W={W} G={G} k={k} hist={with_hist}: worst cost difference {worst:.2f} ulp; tied neighbours {ties}")
    assert shared3 >= 1 and (ties > 0 or W // G == 1)


@pytest.mark.parametrize("W,k", [(4, 4), (6, 5), (8, 8), (1, 1)])
def test_one_group_is_the_plain_selection_bit_for_bit(W, k):
    """G = 1, lambda = 0 reproduces, bit for bit, every output that the single-beam selection kernel of the parent commit (its
    two entry points, without and with paths; the fixture's note names the commit) wrote for the same inputs on an MI355X"""
    from tests._util import GOLDEN
    want = np.load(os.path.join(GOLDEN, "beam_select_parent.npz"))
    tok, cost, done, p, ids = D.hand_fringes(W, 1, k)
    hist_len, ld = 5, 9
    hist = _hist_for(tok, hist_len, ld)
    for with_hist in (False, True):
        got = _select_groups(tok, cost, done, p, ids, 1, 0.0, hist if with_hist else None, hist_len)
        pre = f"W{W}_k{k}_{'hist' if with_hist else 'plain'}_"
        assert sorted(key[len(pre):] for key in want.files if key.startswith(pre)) == sorted(got)
        for key, arr in got.items():
            arr = arr.view(np.int32) if key == "cost" else arr
            assert arr.dtype == want[pre + key].dtype and np.array_equal(arr.reshape(-1), want[pre + key].reshape(-1)), (with_hist, key)


def test_one_group_leaves_the_call_path_untouched(monkeypatch):
    """num_beam_groups = 1, diversity_penalty = 0 are the calls of before: the selection is never reached with G != 1 or a penalty,
    the attention search never with num_groups != 1, and the results are the same"""
    from showtell_amd import _lib, beam, rnn_attn

    real = _lib.lib()

    class Guard:
        def st_beam_select(self, *a):
            if a[7] != 1 or a[10] != 0.0:                                          # G, diversity_penalty
                raise AssertionError("st_beam_select reached with one group")
            return real.st_beam_select(*a)

        def st_attn_beam_search(self, *a):
            opts = a[14]
            if opts is not None and opts._obj.num_groups != 1:
                raise AssertionError("st_attn_beam_search reached with one group")
            return real.st_attn_beam_search(*a)

        def __getattr__(self, name):
            return getattr(real, name)

    for case in ("plain-gru-fp32", "attn-lstm-fp32"):
        name, _ = CASES[case]
        kind, _, W, G, B, _ = D.DECODERS[name]
        m, feat = _model(case), K.features(kind, B).cuda()
        for kw in (dict(), dict(suppress_tokens=[], length_penalty=0.7)):
            before = m.beam_search(feat, W, 3, T, START, END, **kw)
            with monkeypatch.context() as mp:
                mp.setattr(beam, "lib", lambda: Guard())
                mp.setattr(rnn_attn, "lib", lambda: Guard())
                after = m.beam_search(feat, W, 3, T, START, END, num_beam_groups=1, diversity_penalty=0.0, **kw)
                with pytest.raises(AssertionError, match="reached with one group"):
                    m.beam_search(feat, W, 3, T, START, END, num_beam_groups=G, **kw)
            assert repr(before) == repr(after) and any(before)
    m, feat = _model("plain-gru-fp32"), K.features("plain", 24).cuda()
    a = beam.beam_search_records(m, feat, 4, T, START, END)
    b = beam.beam_search_records(m, feat, 4, T, START, END, num_beam_groups=1, diversity_penalty=0.0)
    assert all(np.array_equal(a[key], b[key]) for key in a) and set(a) == set(b)


# ====================================================================================================================
# (c), (d), (e) the searches
# ====================================================================================================================

@pytest.mark.parametrize("case", [c for c in CASES if c.endswith("fp32")])
def test_without_penalty_every_group_repeats_group_0(case):
    from showtell_amd.beam import group_records
    name, _ = CASES[case]
    G = D.DECODERS[name][3]
    _, rec = _search(case, 0.0, D.NONE)
    g0 = group_records(rec, 0, G)
    assert np.isfinite(g0["cost"]).sum() > T * rec["tok"].shape[1] // 2
    worst = 0.0
    for g in range(1, G):
        r = group_records(rec, g, G)
        for key in ("tok", "par", "end"):
            assert np.array_equal(r[key], g0[key]), (g, key)
        fin = np.isfinite(g0["cost"])
        assert np.array_equal(np.isfinite(r["cost"]), fin)
        worst = max(worst, float(np.abs(r["cost"][fin].astype(np.float64) - g0["cost"][fin]).max()))
    print(f"MEASURE {case} lam=0: worst cost difference between a group and group 0 {worst:.2e}")
    assert worst <= T * 4 * FLOOR[case]


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("lam", D.LAMBDAS)
@pytest.mark.parametrize("case", list(CASES))
def test_diverse_records_follow_the_oracle(case, lam, setting):
    name, dtype = CASES[case]
    kind, _, W, G, B, _ = D.DECODERS[name]
    cons = SETTINGS[setting]
    hyps, rec = _records(case, lam, setting)
    hist = rec.get("hist")
    if setting == "all" or kind == "attn":
        assert hist is not None and hist.shape == (B, W, T + 1)                 # the paths the search kept
    check_records(rec, D.oracle(name, storage=dtype == "bf16"), 4 * FLOOR[case], f"{case} lam={lam} {setting}", cons, G, lam, hist=hist)
    assert len(hyps) == B and all(len(h) == G for h in hyps)
    for per_image in hyps:
        for group in per_image:
            assert len(group) <= 1
            for h in group:
                seq = h[0]
                assert seq[0] == START and seq[-1] == END and len(seq) - 2 >= cons[0] and not set(seq[1:]) & set(cons[2] or ())
                if cons[1]:
                    grams = [tuple(seq[i:i + cons[1]]) for i in range(len(seq) - cons[1] + 1)]
                    assert len(grams) == len(set(grams)), (seq, "an n-gram repeats")


@pytest.mark.parametrize("case", ["plain-gru-fp32", "plain-lstm-fp32", "attn-gru-fp32", "attn-lstm-bf16", "plain-gru-g8-fp32"])
def test_returned_groups_are_the_replayed_slices(case):
    """beam_search(num_beam_groups=G) returns, per image, replay_hypotheses of each sliced group, with and without a length penalty;
    the attention decoders with their alphas"""
    from showtell_amd.beam import group_records, replay_hypotheses
    name, _ = CASES[case]
    kind, _, W, G, B, _ = D.DECODERS[name]
    n_hyp = 0
    name_ok = name != "plain-gru-g8"          # the float64 oracle harvests a caption for every image of the other cases at lam = 0.5
    for setting in SETTINGS:
        for a in (0.0, 0.7):
            for nh in (1, 3):
                hyps, rec = _search(case, 0.5, SETTINGS[setting], nh, alphas=True, length_penalty=a)
                assert ("alpha" in rec) == (kind == "attn")
                assert len(hyps) == B
                if setting == "free" and name_ok:                 # most images harvest: the replay is compared on real hypotheses
                    assert sum(any(len(x) for x in h) for h in hyps) >= B // 2
                for g in range(G):
                    r = group_records(rec, g, G)
                    want = replay_hypotheses(r["tok"], r["cost"], r["par"], r["end"], nh, r.get("alpha"), a)
                    for b in range(B):
                        got = hyps[b][g]
                        assert [(h[0], h[1]) for h in got] == [(h[0], h[1]) for h in want[b]] and len(got) <= nh
                        if kind == "attn":
                            assert all(torch.equal(x[2], y[2]) and x[2].shape[0] == len(x[0]) - 1 for x, y in zip(got, want[b]))
                        n_hyp += len(got)
    assert n_hyp > 0


# ====================================================================================================================
# (f) loud failures
# ====================================================================================================================

def test_group_arguments_are_rejected_with_the_device_untouched(monkeypatch):
    from showtell_amd import beam, rnn_attn
    from tests.test_diverse_beam_inputs import BAD_GROUPS

    def touched():
        raise AssertionError("the library was reached")

    cases = ("plain-gru-fp32", "plain-lstm-fp32", "attn-gru-fp32", "attn-lstm-fp32")
    models = {case: (_model(case), K.features(D.DECODERS[CASES[case][0]][0], 3).cuda()) for case in cases}
    monkeypatch.setattr(beam, "lib", touched)
    monkeypatch.setattr(rnn_attn, "lib", touched)
    for case in cases:
        kind = D.DECODERS[CASES[case][0]][0]
        m, feat = models[case]
        for bad in BAD_GROUPS:
            with pytest.raises(ValueError):
                m.beam_search(feat, **bad)
        if kind == "plain":
            for bad in (dict(beam_width=10, num_beam_groups=2), dict(beam_width=4, num_beam_groups=2, on_device=False)):
                with pytest.raises(ValueError, match="on the device only"):
                    beam.beam_search(m, feat, **bad)
            with pytest.raises(ValueError, match="on the device only"):
                beam.beam_search_host(m, feat, 4, num_beam_groups=2)
        with pytest.raises(AssertionError, match="the library was reached"):
            m.beam_search(feat, 4, num_beam_groups=2, diversity_penalty=0.5)      # the guard works: a legal call reaches it


def test_c_entry_points_refuse_and_leave_the_outputs_alone():
    from showtell_amd._lib import ShowTellHipError, check, lib
    from showtell_amd.rnn import _cp, _stream
    tok, cost, done, p, ids = D.hand_fringes(6, 2, 6, B=4)
    hist = _hist_for(tok, 5, 9)
    for G, lam, k, h, hl in ((4, 0.5, 6, None, 0), (0, 0.5, 6, None, 0), (2, -1.0, 6, None, 0), (2, float("nan"), 6, None, 0),
                             (2, float("inf"), 6, None, 0), (2, 0.5, 6, hist, 0), (2, 0.5, 6, hist, 9)):
        with pytest.raises(ShowTellHipError):
            _select_groups(tok, cost, np.zeros((4, max(G, 1)), np.uint8), p, ids, G, lam, h, hl, k)
    tok8, cost8, done8, p8, ids8 = D.hand_fringes(12, 2, 6, B=2)
    with pytest.raises(ShowTellHipError):                                          # W * k = 72
        _select_groups(tok8, cost8, done8, p8, ids8, 2, 0.5)
    with pytest.raises(ShowTellHipError):                                          # k > W
        _select_groups(tok[:, :3].copy(), cost[:, :3].copy(), done[:, :1].copy(), p[:12].copy(), ids[:12].copy(), 1, 0.0)
    # a refused call writes nothing
    dev = "cuda"
    outs = [torch.full((4, 6), -7, device=dev, dtype=torch.long), torch.full((4, 6), -7.0, device=dev),
            torch.full((4, 6), -7, device=dev, dtype=torch.int32), torch.full((4, 6), 7, device=dev, dtype=torch.uint8),
            torch.full((24,), -7, device=dev, dtype=torch.int32)]
    t_done = torch.full((8,), 5, device=dev, dtype=torch.uint8)
    ins = [torch.from_numpy(x).to(dev) for x in (tok, cost)] + [t_done] + [torch.from_numpy(x).to(dev) for x in (p, ids)]
    for G, lam in ((4, 0.5), (2, -1.0), (2, float("nan"))):
        with pytest.raises(ShowTellHipError):
            check(lib().st_beam_select(*[_cp(x) for x in ins], 4, 6, G, 6, END, lam, *[_cp(x) for x in outs], None, None, 0, 0,
                                       _stream()), "st_beam_select")
    torch.cuda.synchronize()
    assert all((x == (7 if x.dtype == torch.uint8 else -7)).all() for x in outs) and (t_done == 5).all()
    # st_attn_beam_search
    from showtell_amd._lib import BeamOpts
    m, feat = _model("attn-gru-fp32"), K.features("attn", 3).cuda()
    prm, keep, featc, B, P = m._decode_inputs(feat)
    W = 6

    def opts(G=1, lam=0.0, keep_paths=1, ngram=0):
        return C.byref(BeamOpts(0, ngram, None, 0, keep_paths, G, lam))

    def planned(max_length, o):
        off = C.c_size_t(77)
        return lib().st_attn_beam_workspace_bytes(C.byref(prm), B, W, max_length, o, C.byref(off)), off.value

    nb, off3 = planned(T, opts(3))
    kept, off1 = planned(T, opts(1))                                               # the constrained search's plan of before
    plain, off0 = planned(T, None)
    assert nb > kept > plain > 0 and off0 == 0 and off1 == off3 == plain + (T & 1) * ((B * W * (T + 1) * 4 + 255) // 256 * 256)
    assert planned(T, opts(1, keep_paths=0)) == (plain, 0)
    assert planned(T, opts(4)) == (0, 0) == planned(T, opts(0))
    assert planned(64, opts(1)) == (0, 0) and planned(64, opts(1, keep_paths=0))[0] == planned(64, None)[0] == plain
    ws = torch.empty(nb, device=dev, dtype=torch.uint8)
    r_tok = torch.full((T + 1, B, W), -7, device=dev, dtype=torch.long); r_cost = torch.full((T + 1, B, W), -7.0, device=dev)
    r_par = torch.full((T + 1, B, W), -7, device=dev, dtype=torch.int32); r_end = torch.full((T, B, W), 7, device=dev, dtype=torch.uint8)
    for G, lam, nbytes, kp, ng, Tn in ((4, 0.5, nb, 1, 0, T), (0, 0.5, nb, 1, 0, T), (3, -1.0, nb, 1, 0, T), (3, float("nan"), nb, 1, 0, T),
                                       (3, 0.5, nb - 256, 1, 0, T), (1, 0.0, nb, 0, 2, T), (1, 0.0, nb, 1, 0, 64)):
        if Tn != T:                                                                # records long enough for the refused call
            big = [torch.full((Tn + 1, B, W), -7, device=dev, dtype=x.dtype) for x in (r_tok, r_cost, r_par)] + \
                  [torch.full((Tn, B, W), 7, device=dev, dtype=torch.uint8)]
        recs = (r_tok, r_cost, r_par, r_end) if Tn == T else big
        with pytest.raises(ShowTellHipError):
            check(lib().st_attn_beam_search(C.byref(prm), _cp(featc), B, W, Tn, START, END, _cp(ws), nbytes, *[_cp(x) for x in recs], None,
                                            opts(G, lam, kp, ng), _stream()), "st_attn_beam_search")
        if Tn != T:
            torch.cuda.synchronize()
            assert all((x == (7 if x.dtype == torch.uint8 else -7)).all() for x in big)
    torch.cuda.synchronize()
    assert (r_tok == -7).all() and (r_cost == -7).all() and (r_par == -7).all() and (r_end == 7).all()


if __name__ == "__main__":
    torch.set_num_threads(8)
    for case_, (name_, dtype_) in CASES.items():
        fl = {f"{lam_}/{s_}": D.floor(name_, dtype_ == "bf16", lam_, c_) for lam_ in D.LAMBDAS for s_, c_ in SETTINGS.items()}
        print(f'    "{case_}": {max(fl.values()):.2e},      # ' + " ".join(f"{c} {v:.1e}" for c, v in fl.items()), flush=True)
