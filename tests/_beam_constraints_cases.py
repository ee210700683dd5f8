"""Shared by test_beam_constraints_inputs.py (CPU) and test_gpu_beam_constraints.py: the ban rule of constrained beam search
in plain Python (written from the three rules of beam.py's docstring, not from the kernel), the decoders and images of the
cases, the float64 oracle's own constrained search, and the walk of a search's records against that oracle.

A node in slot (b, w) of fringe t has the path s_0 .. s_t (s_0 = <start>), read along `par`.  A successor v is banned iff
  1. v is suppressed, or
  2. v == <end> and t < min_length, or
  3. g >= 1 and s[i .. i+g-2] == s[t-g+2 .. t] and s[i+g-1] == v for some 0 <= i <= t-g+1.
"""
import numpy as np
import torch

from oracle import restatement as R

START, END = 1, 2
E = H = 64
L, V, T = 2, 600, 14
HOT = slice(10, 16)            # six words every image likes: what makes repeats common

# the constraint sets of every case: (min_length, no_repeat_ngram_size, suppress).  g1s and g2s are g1 and g2 on a decoder that
# wants <start> again (START_BOOST on its bias): only there does s_0, the root of every path, decide a ban
SUPPRESS5 = [10, 11, 12, 0, 1]                                   # three hot words, <pad> and <start>
CONSTRAINTS = {"g1": (0, 1, None), "g2": (0, 2, None), "g3": (0, 3, None), "min6": (6, 0, None), "sup5": (0, 0, SUPPRESS5),
               "all": (6, 3, SUPPRESS5), "g1s": (0, 1, None), "g2s": (0, 2, None)}
START_BOOST = {"g1s": 6.0, "g2s": 6.0}

# (boost of <end>'s bias, boost of the hot words' bias) per decoder and constraint set (g1s, g2s: those of g1, g2), searched on the CPU so that the float64
# oracle alone meets the input conditions (test_beam_constraints_inputs.py asserts them): a constraint bites only where the model
# wants what it bans -- <end> early for min_length, repeats for n-gram blocking.  A plain sharpened random decoder does not.
INPUTS = {
    ("plain", "gru", 600): dict(g1=(2.25, 3.0), g2=(3.5, 4.0), g3=(5.0, 5.0), min6=(5.0, 4.0), sup5=(2.25, 3.0), all=(3.25, 4.0)),
    ("plain", "lstm", 600): dict(g1=(3.0, 3.0), g2=(3.75, 4.0), g3=(3.25, 4.0), min6=(3.5, 4.0), sup5=(2.75, 3.0), all=(2.5, 3.0)),
    ("plain", "gru", 2056): dict(g1=(3.0, 3.0), g2=(5.5, 5.0), g3=(6.75, 5.0), min6=(7.0, 5.0), sup5=(4.25, 5.0), all=(5.5, 4.0)),
    ("attn", "gru", 600): dict(g1=(4.25, 3.0), g2=(3.75, 4.0), g3=(5.5, 5.0), min6=(6.0, 4.0), sup5=(5.0, 4.0), all=(5.0, 5.0)),
    ("attn", "lstm", 600): dict(g1=(2.5, 3.0), g2=(2.75, 3.0), g3=(4.0, 4.0), min6=(4.25, 4.0), sup5=(2.0, 3.0), all=(3.75, 3.0)),
}

_CACHE = {}


def _bf16(t):
    return t.bfloat16().float()


# ====================================================================================================================
# the rule
# ====================================================================================================================

def banned_tokens(path, min_length=0, g=0, suppress=None, end_id=END):
    """the set of banned successors of a node with the path s_0 .. s_t (a list of t + 1 ids)"""
    t = len(path) - 1
    out = set(suppress or ())
    if t < min_length:
        out.add(end_id)
    if g >= 1:
        tail = list(path[t - g + 2:t + 1]) if g > 1 else []
        for i in range(0, t - g + 2):
            if list(path[i:i + g - 1]) == tail:
                out.add(path[i + g - 1])
    return out


def banned_brute_force(path, vocab, min_length=0, g=0, suppress=None, end_id=END):
    """the same set by trying every v: is the last n-gram of path + [v] one of the n-grams of the path?"""
    t = len(path) - 1
    out = set()
    grams = {tuple(path[i:i + g]) for i in range(len(path) - g + 1)} if g >= 1 else set()
    for v in range(vocab):
        new = list(path) + [v]
        if (suppress and v in suppress) or (v == end_id and t < min_length) or (g >= 1 and len(new) >= g and tuple(new[-g:]) in grams):
            out.add(v)
    return out


def slot_paths(tok, par, t):
    """paths (B, W, t + 1) of the slots of fringe t, read along par (an empty slot: zeros)"""
    B, W = tok.shape[1:]
    out = np.zeros((B, W, t + 1), np.int64)
    w = np.broadcast_to(np.arange(W), (B, W)).copy()
    ok = np.ones((B, W), bool)
    for s in range(t, -1, -1):
        bb = np.arange(B)[:, None]
        ok &= w >= 0
        ws = np.where(ok, w, 0)
        out[:, :, s] = np.where(ok, tok[s][bb, ws], 0)
        w = np.where(ok, par[s][bb, ws], -1) if s > 0 else w
    filled = par[t] >= 0 if t > 0 else np.broadcast_to(np.arange(W) == 0, (B, W))
    return np.where(filled[:, :, None], out, 0)


def ban_mask(paths, vocab, cons, rule=banned_tokens):
    """bool (B * W, V): the ban set of every slot of a fringe"""
    m, g, sup = cons
    B, W, _ = paths.shape
    out = np.zeros((B * W, vocab), bool)
    for r, p in enumerate(paths.reshape(B * W, -1).tolist()):
        ids = [v for v in rule(p, m, g, sup) if 0 <= v < vocab]
        out[r, ids] = True
    return out


# ====================================================================================================================
# decoders, images, the float64 oracle
# ====================================================================================================================

def decoder_params(kind, cell, vocab=V, cname="all"):
    """bf16-representable parameters of the decoder that constraint set `cname` is tested on: a x10 vocabulary projection, <end>
    and the six hot words raised by INPUTS, <start> by START_BOOST"""
    key = ("params", kind, cell, vocab, cname)
    if key not in _CACHE:
        attn = dict(F=72, A=40) if kind == "attn" else None
        p = {k: v.clone() for k, v in R.init_decoder_params(E, H, vocab, L, cell, seed=9, attn=attn).items()}
        p["linear.weight"] *= 10.0
        e, hot = INPUTS[(kind, cell, vocab)][cname[:2] if cname in START_BOOST else cname]
        p["linear.bias"][END] += e
        p["linear.bias"][HOT] += hot
        p["linear.bias"][START] += START_BOOST.get(cname, 0.0)
        _CACHE[key] = {k: (_bf16(v) if v.is_floating_point() else v) for k, v in p.items()}
    return _CACHE[key]


def features(kind, B):
    g = torch.Generator().manual_seed(9)
    return _bf16(torch.randn(B, E, generator=g) if kind == "plain" else torch.randn(B, 72, 9, generator=g).abs())


class Oracle:
    """oracle/restatement.py's teacher-forced beam steps of one decoder on one batch, in `dt` arithmetic"""

    def __init__(self, kind, cell, params, feat, W, storage, dt=torch.float64):
        self.kind, self.cell, self.W, self.storage, self.B = kind, cell, W, storage, feat.shape[0]
        self.p = {k: v.to(dt) if v.is_floating_point() else v for k, v in params.items()}
        self.V = params["linear.weight"].shape[0]
        with torch.no_grad():
            if kind == "plain":
                self.ctx, self.state0 = None, R.rnn_beam_init_bf16_storage(self.p, feat.to(dt), W, cell, storage)
            else:
                self.ctx, self.state0 = R.attn_beam_init_bf16_storage(self.p, feat.to(dt), W, cell, storage)

    def step(self, tok, state, par_next=None):
        with torch.no_grad():
            if self.kind == "plain":
                return R.rnn_beam_step_bf16_storage(self.p, tok, state, par_next, self.cell, self.storage)
            logp, _, state = R.attn_beam_step_bf16_storage(self.p, self.ctx, tok, state, par_next, self.cell, self.storage)
            return logp, state

    def follow(self, rec):
        """yields (t, log_softmax rows (B*W, V)) of every iteration, teacher-forced on the records"""
        state = self.state0
        for t in range(rec["end"].shape[0]):
            logp, state = self.step(rec["tok"][t], state, rec["par"][t + 1])
            yield t, logp

    def free_run(self, cons, Tn=T, rule=banned_tokens, after_cut=False, renormalise=False, own_slot_paths=False):
        """R.beam_free_run under constraints: a node's successors are its W most probable UNBANNED entries at the model's own
        log p.  `rule`, `after_cut` (bans applied to the unconstrained top W) and `renormalise` (log p over the unbanned set)
        and `own_slot_paths` (slot w extends the path slot w had, not its parent's) are the seeded faults of test_beam_constraints_inputs.  Returns the records, with `top_banned` [T][B][W] (at least one of
        the unconstrained top W is banned) and `mass_banned` [T][B][W] (probability mass of the ban set) of every slot, and `gap` [T][B], the cost
        distance between the last candidate taken into the fringe and the first one left out."""
        B, W, Vn = self.B, self.W, self.V
        tok = np.zeros((Tn + 1, B, W), np.int64); tok[0, :, 0] = START
        cost = np.full((Tn + 1, B, W), np.inf); cost[0, :, 0] = 0
        par = np.full((Tn + 1, B, W), -1, np.int32)
        end = np.zeros((Tn, B, W), np.uint8)
        top_banned, mass_banned = np.zeros((Tn, B, W), bool), np.zeros((Tn, B, W))
        live_rec = np.zeros((Tn, B, W), bool)
        gap = np.full((Tn, B), np.inf)
        done = np.zeros(B, bool)
        state = self.state0
        k = min(W, Vn)
        own = np.zeros((B, W, Tn + 1), np.int64); own[:, :, 0] = START
        for t in range(Tn):
            logp, new = self.step(tok[t], state)
            logp = logp.double()
            own[:, :, t] = tok[t]
            ban = torch.from_numpy(ban_mask(own[:, :, :t + 1] if own_slot_paths else slot_paths(tok, par, t), Vn, cons, rule))
            top_banned[t] = ban.gather(1, torch.topk(logp, k, dim=1).indices).any(1).view(B, W).numpy()
            mass_banned[t] = (logp.exp() * ban).sum(1).view(B, W).numpy()
            if renormalise:
                logp = logp - torch.logsumexp(logp.masked_fill(ban, -np.inf), 1, keepdim=True)
            if after_cut:
                tv, ti = torch.topk(logp, k, dim=1)
                tv = tv.masked_fill(ban.gather(1, ti), -np.inf)
            else:
                tv, ti = torch.topk(logp.masked_fill(ban, -np.inf), k, dim=1)
            tv, ti = tv.numpy(), ti.numpy()
            occupied = np.isfinite(cost[t])
            ended = occupied & (tok[t] == END) & ~done[:, None]
            live = occupied & ~ended & ~done[:, None]
            done |= ~live.any(1)
            live &= ~done[:, None]
            end[t], live_rec[t] = ended, live
            cand = cost[t][:, :, None] - tv[:, ::-1].reshape(B, W, k)
            flat = np.where(live[:, :, None], cand, np.inf).reshape(B, W * k)
            order = np.argsort(flat, axis=1, kind="stable")
            if W * k > W:                                                         # how far the first candidate left out lies above the last one taken
                two = np.take_along_axis(flat, order[:, W - 1:W + 1], 1)
                with np.errstate(invalid="ignore"):
                    gap[t] = np.where(np.isfinite(two[:, 1]), two[:, 1] - two[:, 0], np.inf)
            order = order[:, :W]
            ncost = np.take_along_axis(flat, order, 1)
            ok = np.isfinite(ncost)
            tok[t + 1] = np.where(ok, np.take_along_axis(ti[:, ::-1].reshape(B, W * k), order, 1), 0)
            par[t + 1] = np.where(ok, order // k, -1)
            cost[t + 1] = np.where(ok, ncost, np.inf)
            state = R.beam_gather_state(new, par[t + 1], W)
        return dict(tok=tok, cost=cost, par=par, end=end, top_banned=top_banned, mass_banned=mass_banned, live=live_rec, gap=gap)


# ====================================================================================================================
# the walk: a search's records against the oracle, teacher-forced on them
# ====================================================================================================================

def check_records(rec, orc, cons, nll_abs, tag, hist=None):
    """Exact: the bookkeeping of test_gpu_beam_bench_shape's check A, no recorded token is banned for its parent, nothing is
    harvested before min_length, and (`hist` [B][W][T+1]) the path of every slot of the last fringe is the one the search kept.
    Within nll_abs: the step cost against the oracle's unmasked -log p (B).  Within sel = 2 nll_abs: every chosen candidate is at
    most sel above the oracle's W-th unbanned candidate, every unbanned candidate more than sel below it is chosen (C).
    Returns the measured worst values; raises AssertionError with the first offenders."""
    tok, cost, par, end = rec["tok"], rec["cost"], rec["par"], rec["end"].astype(bool)
    Tn, B, W = end.shape
    m_len = cons[0]
    sel = 2 * nll_abs
    assert tok.shape == cost.shape == par.shape == (Tn + 1, B, W)
    assert (tok[0, :, 0] == START).all() and (cost[0, :, 0] == 0).all() and np.isinf(cost[0, :, 1:]).all() and (par[0] == -1).all()
    done = np.zeros(B, bool)
    m = dict(nll=0.0, chosen=-np.inf, missed=-np.inf, live=0, checked=0, harvested=0)
    bad = []
    for t, logp in orc.follow(rec):
        logp = logp.double()
        Vn = logp.shape[1]
        c_t = cost[t].astype(np.float64)
        occupied = np.isfinite(c_t)
        ended = occupied & (tok[t] == END) & ~done[:, None]
        assert np.array_equal(end[t], ended), (tag, t, "harvest flags")
        assert not (ended.any() and t <= m_len), (tag, t, "harvested before min_length words")
        m["harvested"] += int(ended.sum())
        live = occupied & ~ended & ~done[:, None]
        done = done | ~live.any(1)
        live &= ~done[:, None]
        n_c, n_p, n_t = cost[t + 1], par[t + 1], tok[t + 1]
        filled = n_p >= 0
        assert np.array_equal(filled, np.isfinite(n_c)), (tag, t, "par = -1 exactly where cost = +inf")
        assert not filled[done].any(), (tag, t, "a finished image has a non-empty slot")
        assert (n_p < W).all() and (n_t[~filled] == 0).all(), (tag, t)
        bb, ww = np.nonzero(filled)
        pw = n_p[bb, ww].astype(np.int64)
        assert live[bb, pw].all(), (tag, t, "the parent of a non-empty slot is a live slot")
        with np.errstate(invalid="ignore"):
            assert (n_c[:, :-1] <= n_c[:, 1:]).all(), (tag, t, "fringe costs ascend")
        assert (n_c[bb, ww] >= cost[t][bb, pw]).all(), (tag, t, "a child costs at least its parent")
        m["live"] += int(live.sum())
        ban = ban_mask(slot_paths(tok, par, t), Vn, cons)                         # (B * W, V)
        # a live image fills every slot for which an unbanned candidate exists
        n_cand = np.where(live, np.minimum(W, Vn - ban.reshape(B, W, Vn).sum(2)), 0).sum(1)
        assert np.array_equal(filled.sum(1), np.minimum(W, n_cand)), (tag, t, "slots filled")
        if bb.size == 0:
            continue
        assert not ban[bb * W + pw, n_t[bb, ww]].any(), (tag, t, "a recorded token is banned for its parent")
        # B
        rows = torch.from_numpy(bb * W + pw)
        nll_o = -logp[rows, torch.from_numpy(n_t[bb, ww])].numpy()
        nll_g = n_c[bb, ww].astype(np.float64) - c_t[bb, pw]
        err = np.abs(nll_g - nll_o) - np.spacing(n_c[bb, ww].astype(np.float32)).astype(np.float64)
        m["checked"] += int(bb.size)
        m["nll"] = max(m["nll"], float(err.max()))
        if err.max() > nll_abs:
            i = int(err.argmax())
            bad.append(("B", t, int(bb[i]), int(ww[i]), float(err[i])))
        # C: the oracle's unbanned candidates of all live parents
        k = min(W, Vn)
        tv, ti = torch.topk(logp.masked_fill(torch.from_numpy(ban), -np.inf), k, dim=1)
        tv, ti = tv.view(B, W, k).numpy(), ti.view(B, W, k).numpy()
        cand = np.where(live[:, :, None], c_t[:, :, None] - tv, np.inf).reshape(B, W * k)
        kth = np.partition(cand, W - 1, axis=1)[:, W - 1]
        over = (c_t[bb, pw] + nll_o) - kth[bb]
        over = np.where(np.isfinite(kth[bb]), over, -np.inf)                      # fewer than W candidates: all are chosen
        m["chosen"] = max(m["chosen"], float(over.max()))
        key = (np.arange(W)[None, :, None] * Vn + ti).reshape(B, W * k)
        chosen = np.where(filled, n_p.astype(np.int64) * Vn + n_t, -1)
        present = (key[:, :, None] == chosen[:, None, :]).any(2)
        with np.errstate(invalid="ignore"):
            below = np.where(present | ~np.isfinite(cand), -np.inf, np.where(np.isfinite(kth), kth, np.inf)[:, None] - cand)
        m["missed"] = max(m["missed"], float(below.max()))
        if over.max() > sel or below.max() > sel:
            bad.append(("C", t, int(bb[int(over.argmax())]), float(over.max()), float(below.max())))
    if hist is not None:
        assert np.array_equal(hist.astype(np.int64), slot_paths(tok, par, Tn)), (tag, "the kept paths are not the paths along par")
    excluded = 1.0 - m["checked"] / max(1, int((par[1:] >= 0).sum()))
    print(f"MEASURE {tag}: |d nll| {m['nll']:.2e} nats; selection: chosen above the W-th {m['chosen']:.2e}, missed below it "
          f"{m['missed']:.2e}; live slots {m['live']}, harvested {m['harvested']}, checked {m['checked']}, excluded share {excluded}")
    assert excluded == 0.0
    assert not bad, (tag, nll_abs, bad[:8])
    return m


def floor(kind, cell, storage, W, B, vocab, cname, Tn=T):
    """|d nll| of the restatement in fp32 against float64 arithmetic, both teacher-forced on the float64 oracle's own
    constrained free run: what any implementation that accumulates in fp32 is off by"""
    params, feat = decoder_params(kind, cell, vocab, cname), features(kind, B)
    o64 = Oracle(kind, cell, params, feat, W, storage)
    rec = o64.free_run(CONSTRAINTS[cname], Tn)
    o32 = Oracle(kind, cell, params, feat, W, storage, torch.float32)
    worst = 0.0
    for (t, l64), (_, l32) in zip(o64.follow(rec), o32.follow(rec)):
        bb, ww = np.nonzero(rec["par"][t + 1] >= 0)
        if bb.size:
            rows = torch.from_numpy(bb * W + rec["par"][t + 1][bb, ww].astype(np.int64))
            col = torch.from_numpy(rec["tok"][t + 1][bb, ww])
            worst = max(worst, float((l64[rows, col].double() - l32[rows, col].double()).abs().max()))
    return worst
