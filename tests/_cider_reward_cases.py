"""CIDEr rewards on the device: the float64 oracle, the numpy replica of the kernel's algorithm (with its seeded faults) and the
cases that tests/test_gpu_cider_reward.py (GPU) and tests/test_cider_reward_inputs.py (CPU) share.  Nothing here needs a GPU.

The score (include/showtell_hip.h, st_cider_reward; evaluation.cider_score is the definition).  A caption's words are its ids
before the first end_id, within its length.  Per caption and order n = 1..4 every distinct n-gram g has tf = its count and
w = tf * (log N - log max(1, df(g))); norm_n = sqrt(sum w^2); len = max(words - 1, 0).  Per candidate, reference and order
val_n = sum over the candidate's distinct g of min(w_c, w_r) * w_r (w_r = 0 if the reference lacks g), divided by norm_c * norm_r
when both are non-zero, times exp(-(len_c - len_r)^2 / (2 sigma^2)), sigma = 6.  Score = 10 * mean_n(sum_refs val_n) / (number
of references of the image).  df and N come from an explicit table (keys, df, N).

`oracle_scores` states that over Counters of id tuples, as evaluation.cider_score does over word tuples; `replica_scores` states it
the way the kernel computes it (packed keys, tf by comparing positions, df by binary search, the first occurrences carrying the
sums) and takes the faults."""
import functools
import math
from collections import Counter

import numpy as np
import torch

from showtell_amd import evaluation as E

END = 2
SIGMA = 6.0
FAULTS = ["miss_idf0", "tf1", "noclip", "no_end", "div_R"]
CASES = ["mixed", "single", "limits", "corpus", "grid"]
BATCH_DF = ["mixed", "single", "limits", "grid"]           # the cases whose table is CiderTable.from_batch of their references


# ---- the cases ----------------------------------------------------------------------------------------------------------------

def _pad(rows, width, fill=0):
    out = torch.full((len(rows), width), fill, dtype=torch.int64)
    for i, r in enumerate(rows):
        out[i, :len(r)] = torch.tensor(r, dtype=torch.int64)
    return out


def _mixed():
    """B = 6, S = 3, T = 14, V = 12 (ids 0 .. 11, <end> = 2): 1 to 5 references of 1 to 11 words per image; the tiny vocabulary
    forces shared n-grams.  Greedy rows of width 9; sample (0, 1) IS the greedy caption of image 0, at another width."""
    rng = np.random.RandomState(5)
    words = [w for w in range(12) if w != END]
    nrefs, B, S, T, Tg = [3, 1, 5, 2, 4, 2], 6, 3, 14, 9
    refs = [[[int(t) for t in rng.choice(words, size=rng.randint(1, 12))] for _ in range(n)] for n in nrefs]
    refs[1] = [[5, 5, 5, 5, 5]]                            # tf > 1 on both sides: the clipping min(w_c, w_r) matters
    refs[3][0] = [7]                                       # a one-word reference: no bigram, length 0
    refs[0][1] = [4, 9, 4, 9, 4, 9, 3, 0, 1, 6, 8]         # 11 words, repeated bigrams
    ids = torch.zeros(B, S, T, dtype=torch.int64)
    lengths = torch.zeros(B, S, dtype=torch.int64)

    def put(b, s, row, length=None):
        ids[b, s, :len(row)] = torch.tensor(row)
        lengths[b, s] = len(row) if length is None else length
    for b in range(B):
        for s in range(S):                                 # by default: a reference of the image, perturbed, then <end>
            r = list(refs[b][s % len(refs[b])])
            for _ in range(2):
                r[rng.randint(len(r))] = int(rng.choice(words))
            r = (r + [int(t) for t in rng.choice(words, size=rng.randint(0, 3))])[:T - 1]
            put(b, s, r + [END])
    put(0, 0, refs[0][1] + [END])                          # a candidate equal to a reference
    put(1, 0, [5, 5, 5, END])                              # 5 5 5 against 5 5 5 5 5
    put(1, 1, [5, 5, 5, 5, 5, 5, 5, END])                  # ... and longer than the reference
    put(2, 0, [END, 4, 9, 4], 4)                           # first token <end>: score exactly 0
    put(3, 1, [7, END, 7, 7, 7, 9, 9], 7)                  # <end> inside the length, junk after it
    put(4, 2, refs[4][0][:6] + [END, 3, 3, 3, 3], 11)      # the same, after a reference's prefix
    put(5, 0, [int(t) for t in rng.choice(words, size=T)]) # never ends: all T tokens are words
    greedy = torch.zeros(B, Tg, dtype=torch.int64)
    for b in range(B):
        r = list(refs[b][0])[:Tg - 1]
        greedy[b, :len(r) + 1] = torch.tensor(r + [END])
        greedy[b, len(r) + 1:] = 6                         # st_rnn_greedy keeps decoding after <end>: junk, not padding
    g0 = [4, 9, 3, 0, 4, 9]
    greedy[0] = torch.tensor(g0 + [END, 6, 6])
    put(0, 1, g0 + [END])
    return dict(references=refs, ids=ids, lengths=lengths, greedy=greedy, table=E.CiderTable.from_batch(refs, END))


def _single():
    """B = 1: log N = 0 and every df is 1, so every weight, score and advantage is exactly 0.0"""
    refs = [[[4, 5, 6, 7], [4, 5, 9]]]
    ids = _pad([[4, 5, 6, 7, END], [9, 9, 4, END, 0]], 6).view(1, 2, 6)
    return dict(references=refs, ids=ids, lengths=torch.tensor([[5, 4]]), greedy=_pad([[4, 5, 9, END]], 5),
                table=E.CiderTable.from_batch(refs, END))


def _limits():
    """B = 2, R = 8 references of 64 words, T = 64, ids up to 65534 (4-grams whose key is negative as int64)"""
    rng = np.random.RandomState(6)
    pool = [0, 1, 3, 65534, 65533, 40000, 32767, 32766, 12345, 7]
    refs = [[[int(t) for t in rng.choice(pool, size=64)] for _ in range(8)] for _ in range(2)]
    refs[1][7] = [65534] * 64
    ids = torch.zeros(2, 2, 64, dtype=torch.int64)
    ids[0, 0] = torch.tensor(refs[0][3])                                   # a 64-word candidate that never ends
    ids[0, 1] = torch.tensor(refs[0][0][:30] + refs[0][5][10:44])
    ids[1, 0] = torch.tensor([65534] * 40 + [END] + [65534] * 23)
    ids[1, 1] = torch.tensor(refs[1][2][:63] + [END])
    greedy = torch.tensor([refs[0][1], refs[1][7]], dtype=torch.int64)
    return dict(references=refs, ids=ids, lengths=torch.full((2, 2), 64), greedy=greedy, table=E.CiderTable.from_batch(refs, END))


def _corpus():
    """A 40-image corpus table and a 4-image batch.  Every corpus reference starts with 7 (df = N: idf 0); id 29 is in no corpus
    caption, so n-grams with it miss the table (idf = log N) -- in candidates and, for image 3, in a reference too."""
    rng = np.random.RandomState(7)
    words = [w for w in range(3, 29)]
    corpus = [[[7] + [int(t) for t in rng.choice(words, size=rng.randint(4, 10))] for _ in range(3)] for _ in range(40)]
    refs = [list(corpus[b]) for b in range(4)]
    refs[3] = refs[3] + [[7, 29, 11, 29, 12]]
    rows = [[list(refs[b][0]), list(refs[b][1][:5]) + [29, 29], [29] + list(refs[b][2][1:])] for b in range(4)]
    rows[3][0] = [7, 29, 11, 4, 12]
    T = 12
    ids = torch.stack([_pad([r[:T - 1] + [END] for r in img], T) for img in rows])
    lengths = torch.tensor([[len(r[:T - 1]) + 1 for r in img] for img in rows])
    return dict(references=refs, ids=ids, lengths=lengths, greedy=None, table=E.CiderTable.from_corpus(corpus, END))


def _grid():
    """B = 130, S = 5, T = 25, V = 50: 130 workgroups of six candidates, five references of 6 to 15 words per image"""
    rng = np.random.RandomState(8)
    B, S, T = 130, 5, 25
    words = [w for w in range(50) if w != END]
    refs = [[[int(t) for t in rng.choice(words, size=rng.randint(6, 16))] for _ in range(5)] for _ in range(B)]
    ids = torch.zeros(B, S, T, dtype=torch.int64)
    lengths = torch.zeros(B, S, dtype=torch.int64)
    for b in range(B):
        for s in range(S):
            r = list(refs[b][s])
            for _ in range(3):
                r[rng.randint(len(r))] = int(rng.choice(words))
            r = r[:T - 1] + [END]
            ids[b, s, :len(r)] = torch.tensor(r)
            lengths[b, s] = len(r)
    greedy = _pad([list(refs[b][0][:8]) + [END] for b in range(B)], 25, fill=9)
    return dict(references=refs, ids=ids, lengths=lengths, greedy=greedy, table=E.CiderTable.from_batch(refs, END))


@functools.lru_cache(maxsize=None)
def case(name):
    c = {"mixed": _mixed, "single": _single, "limits": _limits, "corpus": _corpus, "grid": _grid}[name]()
    c["name"] = name
    return c


def candidate_rows(c):
    """[(b, column, ids row as a list, length)] of every candidate of the case: the S samples, then the greedy caption (column S)"""
    B, S, T = c["ids"].shape
    out = []
    for b in range(B):
        for s in range(S):
            out.append((b, s, c["ids"][b, s].tolist(), int(c["lengths"][b, s])))
        if c["greedy"] is not None:
            out.append((b, S, c["greedy"][b].tolist(), c["greedy"].shape[1]))
    return out


def cut(row, length, end_id=END):
    out = []
    for t in row[:length]:
        if t == end_id:
            break
        out.append(int(t))
    return out


# ---- the oracle -----------------------------------------------------------------------------------------------------------------

def _counts(words):
    c = Counter()
    for n in range(1, 5):
        for i in range(len(words) - n + 1):
            c[tuple(words[i:i + n])] += 1
    return c


def _vector(words, dfmap, log_docs):
    vec, norm, length = [dict() for _ in range(4)], [0.0] * 4, 0
    for g, tf in _counts(words).items():
        k = len(g) - 1
        w = float(tf) * (log_docs - np.log(max(1.0, float(dfmap.get(g, 0)))))
        vec[k][g] = w
        norm[k] += w * w
        if k == 1:
            length += tf
    return vec, [np.sqrt(v) for v in norm], length


def oracle_score(words, refs, dfmap, log_docs, sigma=SIGMA):
    """one candidate (a word list) against the references (word lists) of its image, in float64"""
    hv, hn, hl = _vector(words, dfmap, log_docs)
    acc = np.zeros(4)
    for r in refs:
        rv, rn, rl = _vector(r, dfmap, log_docs)
        delta = float(hl - rl)
        val = np.zeros(4)
        for k in range(4):
            for g, w in hv[k].items():
                rw = rv[k].get(g, 0.0)
                val[k] += min(w, rw) * rw
            if hn[k] != 0 and rn[k] != 0:
                val[k] /= hn[k] * rn[k]
            val[k] *= np.e ** (-(delta ** 2) / (2 * sigma ** 2))
        acc += val
    return float(np.mean(acc) / len(refs) * 10.0)


def table_dict(table):
    return {E.unpack_ngram(k): int(d) for k, d in zip(table.keys.tolist(), table.df.tolist())}


@functools.lru_cache(maxsize=None)
def oracle_scores(name):
    """(B, S + 1) float64, column S the greedy caption's (0 without one): computed once per case and shared"""
    c = case(name)
    B, S, _ = c["ids"].shape
    dfmap, log_docs = table_dict(c["table"]), np.log(float(c["table"].num_docs))
    refs = [[cut(r, len(r)) for r in image] for image in c["references"]]
    out = np.zeros((B, S + 1))
    for b, col, row, length in candidate_rows(c):
        out[b, col] = oracle_score(cut(row, length), refs[b], dfmap, log_docs)
    out.setflags(write=False)
    return out


def cider_score_scores(name):
    """The same array from evaluation.cider_score itself (document frequencies over the images of the call): one call per column"""
    c = case(name)
    B, S, _ = c["ids"].shape
    gts = {b: [E._id_string(r, END) for r in refs] for b, refs in enumerate(c["references"])}
    out = np.zeros((B, S + 1))
    for col in range(S + (c["greedy"] is not None)):
        rows = c["ids"][:, col] if col < S else c["greedy"]
        lens = c["lengths"][:, col].tolist() if col < S else [c["greedy"].shape[1]] * B
        res = {b: [E._id_string(rows[b, :lens[b]].tolist(), END)] for b in range(B)}
        out[:, col] = E.cider_score(gts, res)[1]
    return out


# ---- the kernel's algorithm in numpy, with the seeded faults ----------------------------------------------------------------------

def _keys_of(words, n):
    """the packed keys of the n-grams at positions 0 .. len - n, uint64"""
    f = (np.asarray(words, dtype=np.int64) + 1).astype(np.uint64)
    m = len(f) - n + 1
    if m <= 0:
        return np.zeros(0, dtype=np.uint64)
    k = f[:m].copy()
    for j in range(1, n):
        k |= f[j:j + m] << np.uint64(16 * j)
    return k


def _entries(words, tkeys, tdf, log_docs, fault):
    """per order: (keys, weights, first-occurrence mask) by position, and the norms"""
    out, norms = [], []
    for n in range(1, 5):
        k = _keys_of(words, n)
        same = k[:, None] == k[None, :]
        tf = same.sum(1)
        first = ~np.tril(same, -1).any(1)
        if fault == "tf1":
            tf = np.ones_like(tf)
        ks = k.view(np.int64)
        at = np.searchsorted(tkeys, ks)
        hit = (at < len(tkeys)) & (tkeys[np.minimum(at, len(tkeys) - 1)] == ks) if len(tkeys) else np.zeros(len(ks), dtype=bool)
        df = np.where(hit, tdf[np.minimum(at, max(len(tkeys) - 1, 0))], 0) if len(tkeys) else np.zeros(len(ks), dtype=np.int64)
        idf = log_docs - np.log(np.maximum(1.0, df.astype(np.float64)))
        if fault == "miss_idf0":
            idf = np.where(hit, idf, 0.0)
        w = tf.astype(np.float64) * idf
        out.append((k, w, first))
        norms.append(math.sqrt(float(sum(x * x for x in w[first]))))
    return out, norms


def replica_scores(name, fault=None):
    """The scores as st_cider_reward forms them, or under one seeded fault:
    'miss_idf0' a table miss treated as idf 0; 'tf1' tf taken as 1; 'noclip' w_c * w_r without the min; 'no_end' <end> does not
    cut a candidate; 'div_R' the sum over references divided by the padded R instead of the image's reference count"""
    c = case(name)
    B, S, _ = c["ids"].shape
    t = c["table"]
    tkeys, tdf, log_docs = t.keys.numpy(), t.df.numpy().astype(np.int64), math.log(float(t.num_docs))
    refs = [[cut(r, len(r)) for r in image] for image in c["references"]]
    R = max(len(r) for r in refs)
    ref_entries = [[_entries(r, tkeys, tdf, log_docs, fault) + (max(len(r) - 1, 0),) for r in image] for image in refs]
    out = np.zeros((B, S + 1))
    for b, col, row, length in candidate_rows(c):
        words = [int(x) for x in row[:length]] if fault == "no_end" else cut(row, length)
        ce, cn = _entries(words, tkeys, tdf, log_docs, fault)
        clen = max(len(words) - 1, 0)
        acc = [0.0] * 4
        for re_, rn, rlen in ref_entries[b]:
            pen = math.exp(-float(clen - rlen) ** 2 / (2 * SIGMA ** 2))
            for n in range(4):
                (ck, cw, cf), (rk, rw, _) = ce[n], re_[n]
                val = 0.0
                for i in np.nonzero(cf)[0]:
                    m = np.nonzero(rk == ck[i])[0]
                    wr = float(rw[m[-1]]) if len(m) else 0.0
                    val += (cw[i] * wr if fault == "noclip" else min(float(cw[i]), wr) * wr)
                if cn[n] != 0 and rn[n] != 0:
                    val /= cn[n] * rn[n]
                acc[n] += val * pen
        out[b, col] = (((acc[0] + acc[1]) + acc[2]) + acc[3]) / 4.0 / (R if fault == "div_R" else len(refs[b])) * 10.0
    return out


def host_advantage(scores, baseline):
    """train.self_critical_advantage on the float32-rounded oracle scores (B, S + 1)"""
    from showtell_amd.train import self_critical_advantage
    r = torch.from_numpy(np.array(scores, dtype=np.float64)).float()          # a copy: the cached oracle array is read-only
    return self_critical_advantage(r[:, :-1], baseline, r[:, -1] if baseline == "greedy" else None)
