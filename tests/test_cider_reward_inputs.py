"""CIDEr rewards on the device, without a GPU: the key codec and the table, the float64 oracle of tests/_cider_reward_cases.py pinned
to evaluation.cider_score and cider_reward, the numpy replica of the kernel's algorithm pinned to the oracle, five seeded faults that
the GPU test's bound must catch, the argument errors (Python and C, the C ones on host buffers: every check precedes the launch)
and the ABI.

`python -m tests.test_cider_reward_inputs` prints the figures."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from showtell_amd import evaluation as E
from tests import _cider_reward_cases as K

SCORE_TOL = 1e-10                       # tests/test_gpu_cider_reward.py: score64 against the oracle
FAULT_MARGIN = 1e-3                     # every seeded fault leaves that bound by at least this much


# ---- the key codec and the table ------------------------------------------------------------------------------------------------

def test_the_key_codec_round_trips():
    rng = np.random.RandomState(1)
    grams = [(0,), (0, 0), (0, 0, 0), (0, 0, 0, 0), (65534,), (65534,) * 4, (1, 2, 3, 4), (32767, 0, 0, 32766), (5, 65534)]
    grams += [tuple(int(t) for t in rng.randint(0, 65535, size=rng.randint(1, 5))) for _ in range(200)]
    for g in grams:
        key = E.pack_ngram(g)
        assert -(1 << 63) <= key < (1 << 63) and key != 0
        assert E.unpack_ngram(key) == g
        assert int(K._keys_of(list(g), len(g)).view(np.int64)[0]) == key           # the numpy packing of the replica agrees
        assert int(E._ngram_keys(np.asarray(g, dtype=np.int64))[-1]) == key        # ... and the table builder's (its last key: the whole g)
    assert E.pack_ngram((0,)) == 1 and E.pack_ngram((0, 0)) == 0x10001 and E.pack_ngram((65534,) * 4) == -1
    assert E.pack_ngram((0, 0, 0, 32767)) < 0                                       # bit 63: the table's order is the SIGNED one


def test_orders_never_collide():
    """(0) differs from (0, 0): a field is id + 1, never 0, so the highest non-zero field gives the order"""
    keys = {E.pack_ngram((0,) * n) for n in range(1, 5)} | {E.pack_ngram((7,) * n) for n in range(1, 5)}
    assert len(keys) == 8
    every = [E.pack_ngram(g) for g in [(a,) for a in range(4)] + [(a, b) for a in range(4) for b in range(4)]
             + [(a, b, c) for a in range(4) for b in range(4) for c in range(4)]]
    assert len(set(every)) == 4 + 16 + 64


@pytest.mark.parametrize("bad", [(), (1, 2, 3, 4, 5), (65535,), (-1,), (3, 70000)])
def test_the_codec_refuses_what_does_not_fit(bad):
    with pytest.raises(ValueError):
        E.pack_ngram(bad)


@pytest.mark.parametrize("name", K.CASES)
def test_the_table_is_sorted_strictly_and_counts_images(name):
    c = K.case(name)
    t = c["table"]
    assert t.keys.dtype == torch.int64 and t.df.dtype == torch.int32 and t.keys.shape == t.df.shape and t.keys.numel() > 0
    assert bool((t.keys[1:] > t.keys[:-1]).all())
    assert int(t.df.min()) >= 1 and int(t.df.max()) <= t.num_docs
    if name in K.BATCH_DF:                                   # df by hand: the images whose references hold the n-gram
        assert t.num_docs == len(c["references"])
        want = {}
        for refs in c["references"]:
            for g in set(g for r in refs for g in K._counts(K.cut(r, len(r)))):
                want[g] = want.get(g, 0) + 1
        assert K.table_dict(t) == want
    if name == "limits":
        assert int(t.keys[0]) < 0                            # 4-grams ending in an id >= 32767 sort first
    if name == "corpus":
        d = K.table_dict(t)
        assert t.num_docs == 40 and d[(7,)] == 40 and (29,) not in d and (7, 29) not in d


def test_the_table_refuses_what_would_make_a_weight_negative_or_a_search_wrong():
    keys, df = torch.tensor([1, 5, 9]), torch.tensor([1, 2, 3], dtype=torch.int32)
    E.CiderTable(keys, df, 3)
    for k, d, n in [(torch.tensor([1, 9, 5]), df, 3), (torch.tensor([1, 5, 5]), df, 3), (keys, df, 2), (keys, torch.tensor([0, 1, 1], dtype=torch.int32), 3),
                    (keys, df.long(), 3), (keys.int(), df, 3), (keys[:2], df, 3), (keys, df, 0), (torch.tensor([0, 5, 9]), df, 3)]:
        with pytest.raises(ValueError):
            E.CiderTable(k, d, n)
    with pytest.raises(ValueError):
        E.CiderTable.from_corpus([])
    for bad in ([[[3, 65535]]], [[[3, -1]]]):
        with pytest.raises(ValueError, match="65534"):
            E.CiderTable.from_batch(bad)
        with pytest.raises(ValueError, match="65534"):
            E.pack_references(bad)
    E.CiderTable.from_batch([[[3, 2, 70000]]])               # past <end>: not a word, not looked at


def test_references_are_packed_as_words_only():
    refs, ref_len, ref_count = E.pack_references([[[4, 5, 2, 9]], [[6], [7, 8, 9], []]])
    assert refs.dtype == ref_len.dtype == ref_count.dtype == torch.int32
    assert refs.tolist() == [[[4, 5, 0], [0, 0, 0], [0, 0, 0]], [[6, 0, 0], [7, 8, 9], [0, 0, 0]]]
    assert ref_len.tolist() == [[2, 0, 0], [1, 3, 0]] and ref_count.tolist() == [1, 3]
    for bad in ([], [[]], [[[3]] * 9], [[[3] * 65]]):
        with pytest.raises(ValueError):
            E.pack_references(bad)
    E.pack_references([[[3]] * 8, [[3] * 64]])


# ---- the oracle and the replica ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", K.BATCH_DF)
def test_the_oracle_with_the_batch_table_is_cider_score(name):
    got, want = K.oracle_scores(name), K.cider_score_scores(name)
    print(f"MEASURE {name}: oracle against evaluation.cider_score max |d| {np.abs(got - want).max():.2e}; scores {want.min():.3f} .. {want.max():.3f}")
    assert np.abs(got - want).max() <= 1e-12


@pytest.mark.parametrize("name", ["mixed", "single", "limits"])
def test_the_batch_table_reproduces_cider_reward(name):
    """cider_reward returns float32: its values are the oracle's, rounded once (1e-12 in float64, asserted above on the same path)"""
    c = K.case(name)
    S = c["ids"].shape[1]
    host = E.cider_reward(c["references"], K.END)(c["ids"], c["lengths"])
    assert host.dtype == torch.float32
    want = K.oracle_scores(name)[:, :S]
    assert np.abs(host.double().numpy() - want).max() <= 2.0 ** -21 + 1e-12      # half a float32 ulp below 16
    exact = torch.from_numpy(K.cider_score_scores(name)[:, :S].astype(np.float32))
    assert torch.equal(host, exact)


@pytest.mark.parametrize("name", K.CASES)
def test_the_replica_of_the_kernel_is_the_oracle(name):
    got, want = K.replica_scores(name), K.oracle_scores(name)
    print(f"MEASURE {name}: replica against the oracle max |d| {np.abs(got - want).max():.2e}")
    assert np.abs(got - want).max() <= 1e-12


def test_the_cases_hold_what_they_are_for():
    m, s = K.oracle_scores("mixed"), K.case("mixed")
    assert K.cut(s["ids"][0, 0].tolist(), int(s["lengths"][0, 0])) == s["references"][0][1]
    assert m[0, 0] >= 10.0 / 3 - 1e-9        # a candidate equal to one of three references: every val_n on that one is 1
    assert m[2, 0] == 0.0                                                           # first token <end>
    assert m[0, 1] == m[0, 3] > 0                                                   # sample (0, 1) is the greedy caption
    assert 0 < m[1, 0] < m[1, 1] or 0 < m[1, 1] < m[1, 0]                           # 5 5 5 and 5 x 7 against 5 x 5: both clipped, unequal
    assert sorted({len(r) for r in s["references"]}) == [1, 2, 3, 4, 5]
    lens = [len(r) for refs in s["references"] for r in refs]
    assert min(lens) == 1 and max(lens) == 11
    assert (K.oracle_scores("single") == 0.0).all()
    lim = K.case("limits")
    assert all(len(r) == 64 for refs in lim["references"] for r in refs) and lim["ids"].max() == 65534 and lim["ids"].shape[2] == 64
    assert K.oracle_scores("limits").max() > 0.5             # of at most 10 / 8: a candidate equal to one of eight references
    assert K.case("grid")["ids"].shape == (130, 5, 25)
    co = K.oracle_scores("corpus")
    assert (co[:, :-1] > 0).all() and K.case("corpus")["greedy"] is None


# ---- seeded faults ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fault", K.FAULTS)
def test_seeded_faults_leave_the_bound(fault):
    moves = {name: float(np.abs(K.replica_scores(name, fault) - K.oracle_scores(name)).max()) for name in ("mixed", "limits", "corpus")}
    print(f"MEASURE fault {fault}: largest move of a score per case {moves}")
    assert moves["mixed"] >= SCORE_TOL + FAULT_MARGIN
    if fault == "miss_idf0":
        assert moves["corpus"] >= SCORE_TOL + FAULT_MARGIN   # where a reference and a candidate share an n-gram the table lacks


# ---- argument errors ------------------------------------------------------------------------------------------------------------------

def _host_reward(name="mixed"):
    c = K.case(name)
    return c, E.cider_reward_device(c["references"], c["table"], K.END, device="cpu")


def test_python_refusals_come_before_the_device_is_touched():
    from showtell_amd import ShowTellHipError
    c, fn = _host_reward()
    ids, lengths, greedy = c["ids"], c["lengths"], c["greedy"]
    assert callable(fn) and hasattr(fn, "advantage")
    bad = [dict(ids=ids[:3], lengths=lengths[:3]),                                 # another batch
           dict(ids=ids, lengths=lengths[:, :2]),
           dict(ids=ids.int(), lengths=lengths), dict(ids=ids, lengths=lengths.float()),
           dict(ids=ids[:, :0], lengths=lengths[:, :0]),                          # S = 0
           dict(ids=torch.zeros(6, 3, 65, dtype=torch.long), lengths=lengths),     # T = 65
           dict(ids=ids, lengths=lengths + 20),                                   # lengths > T
           dict(ids=ids, lengths=lengths, baseline="median"),
           dict(ids=ids, lengths=lengths, baseline="greedy"),                     # no greedy ids
           dict(ids=ids[:, :1], lengths=lengths[:, :1], baseline="mean"),          # mean with S = 1
           dict(ids=ids, lengths=lengths, baseline="greedy", greedy_ids=greedy[:4]),
           dict(ids=ids, lengths=lengths, baseline="greedy", greedy_ids=torch.zeros(6, 65, dtype=torch.long))]
    for kw in bad:
        kw.setdefault("baseline", None)
        with pytest.raises(ValueError):
            fn.advantage(**kw)
    with pytest.raises(ShowTellHipError):                    # valid arguments get past the checks, to the error of a CPU tensor
        fn(ids, lengths)
    with pytest.raises(ShowTellHipError):
        fn.advantage(ids, lengths, "greedy", greedy)
    with pytest.raises(ValueError):
        E.cider_reward_device(c["references"], table="batch", device="cpu")
    with pytest.raises(ValueError):
        E.cider_reward_device(c["references"], end_id=70000, device="cpu")


C_REFUSALS = {                                               # name: (overrides of the valid call, a word of the message)
    "R = 0": (dict(R=0), "R must be"), "R = 9": (dict(R=9), "R must be"), "Tr = 65": (dict(Tr=65), "reference rows"),
    "S = 0": (dict(S=0), "S must be"), "T = 65": (dict(T=65), "candidate rows"), "T = 0": (dict(T=0), "candidate rows"),
    "Tg = 65": (dict(Tg=65), "greedy rows"), "baseline 3": (dict(baseline=3), "baseline must be"),
    "mean with S = 1": (dict(S=1, baseline=2), "needs S >= 2"), "greedy without ids": (dict(greedy=False, baseline=1), "needs greedy_ids"),
    "sigma 0": (dict(sigma=0.0), "sigma"), "log N < 0": (dict(logn=-1.0), "log"), "log N NaN": (dict(logn=float("nan")), "log"),
    "end_id": (dict(end_id=65535), "end_id"), "B = 0": (dict(B=0), "B must be"),
}


def c_call(L, p, greedy=True, B=2, R=3, Tr=8, S=3, T=10, Tg=9, baseline=1, sigma=6.0, logn=1.0, end_id=2, K_=4, out=None):
    """st_cider_reward on the buffer `p` for every input; `out` = (score64, reward, advantage) pointers"""
    out = out or (p, p, p)
    return L.st_cider_reward(p, p, K_, logn, p, p, p, B, R, Tr, p, p, S, T, p if greedy else None, Tg, end_id, sigma, baseline,
                             out[0], out[1], out[2], None)


@pytest.mark.parametrize("what", sorted(C_REFUSALS))
def test_the_c_entry_point_refuses_ahead_of_any_launch(what):
    """host buffers: the checks precede the launch, so nothing is read or written"""
    from showtell_amd import _lib
    L = _lib.lib()
    host = np.full(4096, 7, dtype=np.int64)
    kw, word = C_REFUSALS[what]
    assert c_call(L, C.c_void_p(host.ctypes.data), **kw) != 0, what
    assert word in L.st_last_error().decode(), (what, L.st_last_error().decode())
    assert (host == 7).all()


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------

def test_the_new_names_are_declared_exported_and_bound():
    from showtell_amd import _lib
    from tests import test_abi as A
    header = A._header_text()
    raw = C.CDLL(_lib.LIB_PATH)
    assert re.search(r"\bint st_cider_reward\(", header)
    assert hasattr(raw, "st_cider_reward") and "st_cider_reward" in _lib._SIGS and callable(_lib.lib().st_cider_reward)
    assert re.search(r"#define ST_CIDER_MAX_REFS %d\b" % E.CIDER_MAX_REFS, header)
    assert re.search(r"#define ST_CIDER_MAX_TOKENS %d\b" % E.CIDER_MAX_TOKENS, header)
    sigs = A._all_sigs()
    assert A.prototype_errors(A.header_prototypes(header), sigs) == []
    assert A.symbol_set_errors(A._header_symbols(), sigs, _lib._EXPERIMENTAL) == []
    args = _lib._SIGS["st_cider_reward"][0]
    assert not any(isinstance(a, type) and issubclass(a, C._Pointer) for a in args)          # flat: no struct by reference
    assert args.count(C.c_double) == 2 and args[-1] is C.c_void_p


if __name__ == "__main__":
    for name in K.CASES:
        o = K.oracle_scores(name)
        print(f"CASE {name}: scores {o.min():.4f} .. {o.max():.4f}, replica max |d| {np.abs(K.replica_scores(name) - o).max():.2e}")
    for fault in K.FAULTS:
        print(f"FAULT {fault}:", {name: "%.3g" % np.abs(K.replica_scores(name, fault) - K.oracle_scores(name)).max() for name in K.CASES})
