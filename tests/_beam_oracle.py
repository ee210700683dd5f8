"""The float64 machinery every beam test shares, on top of oracle/restatement.py: nothing here needs a GPU.

  StepOracle      the teacher-forced storage restatement of one decoder on one batch over fixed (image, slot) rows b * W + w: `step`,
                  `follow` (the walk along given records), `free_run` (R.beam_free_run, the only fringe selection) and, for the
                  W = 1 walkers, `start`
  banned_tokens, ban_mask, slot_paths    the ban rule of constrained beam search in plain Python and the paths it reads
  check_records   a search's records walked by the oracle: the statements below, for plain, constrained and diverse searches
  beam_distance   two oracles walking the same records: what a bound of check_records is four times of

The walk.  A free-running comparison cannot be tight (two correct searches pick different fringes somewhere), so the oracle walks the
search's OWN records: iteration t is teacher-forced on tok[t], the oracle's state of slot (b, w) at t + 1 is its own state of slot
(b, par[t + 1][b][w]) after that step, never a value from the search.

The ban rule.  A node in slot (b, w) of fringe t has the path s_0 .. s_t (s_0 = <start>), read along `par`.  A successor v is banned iff
  1. v is suppressed, or
  2. v == <end> and t < min_length, or
  3. g >= 1 and s[i .. i+g-2] == s[t-g+2 .. t] and s[i+g-1] == v for some 0 <= i <= t-g+1.
"""
import numpy as np
import torch

from oracle import restatement as R

START, END = 1, 2
NONE = (0, 0, None)         # no constraints: (min_length, no_repeat_ngram_size, suppress)
ALPHA_SUM = 1e-5            # |sum - 1| of an fp32 softmax over 49 entries: 49 roundings of 6e-8 and the division; 1.7e-7


class StepOracle:
    """oracle/restatement.py's teacher-forced beam steps of one decoder (`kind` "plain" or "attn") on one batch, in `dt` arithmetic,
    rounded to bf16 where the bf16 kernels store with `storage`.  `step_fn(orc, tok (B, W), state) -> (logp, alpha or None, new
    state)` puts a cases module's own (faulted) step in place of R's."""

    def __init__(self, kind, cell, params, feat, W, storage, dt=torch.float64, step_fn=None):
        self.kind, self.cell, self.W, self.storage, self.step_fn = kind, cell, W, storage, step_fn
        self.p = {k: v.to(dt) if v.is_floating_point() else v for k, v in params.items()}
        self.feat = feat.to(dt)
        self.B, self.V = feat.shape[0], params["linear.weight"].shape[0]
        with torch.no_grad():
            if kind == "plain":
                self.ctx, self.state0 = None, R.rnn_beam_init_bf16_storage(self.p, self.feat, W, cell, storage)
            else:
                self.ctx, self.state0 = R.attn_beam_init_bf16_storage(self.p, self.feat, W, cell, storage)

    @torch.no_grad()
    def start(self):
        """For a W = 1 walker.  Plain: (logits of the image-feature step (B, V), the state after it); attention: (None, the root
        state), the first step being fed <start>."""
        if self.kind != "plain":
            return None, self.state0
        p = self.p
        h = self.feat.new_zeros(R.num_layers_of(p), self.B, p["unit.weight_hh_l0"].shape[1])
        top, h, c = R._cells_storage(p, R._store(self.feat, self.storage), h, None if self.cell == "gru" else h, self.cell, self.storage)
        return top @ p["linear.weight"].t() + p["linear.bias"], (h, c)

    @torch.no_grad()
    def step(self, tok, state, par_next=None):
        """(log_softmax rows (B*W, V), alpha (B*W, P) or None, new state); with `par_next` (the recorded par[t + 1]) the new state is
        already that of iteration t + 1"""
        if self.step_fn is not None:
            logp, alpha, new = self.step_fn(self, tok, state)
        elif self.kind == "plain":
            (logp, new), alpha = R.rnn_beam_step_bf16_storage(self.p, tok, state, None, self.cell, self.storage), None
        else:
            logp, alpha, new = R.attn_beam_step_bf16_storage(self.p, self.ctx, tok, state, None, self.cell, self.storage)
        return logp, alpha, (new if par_next is None else R.beam_gather_state(new, par_next, self.W))

    def follow(self, rec):
        """yields (t, logp, alpha or None) of every iteration, teacher-forced on the records; one block alive at a time.  (No
        torch.no_grad() around the yields: two of these generators are walked in step, and a suspended one would hold it.)"""
        state = self.state0
        for t in range(rec["end"].shape[0]):
            logp, alpha, state = self.step(rec["tok"][t], state, rec["par"][t + 1])
            yield t, logp, alpha
            del logp, alpha

    def free_run(self, T, **hooks):
        """the oracle's own search: R.beam_free_run (its `cost_dtype`, `keep`, `candidates` and `gather_par`) from the root state"""
        return R.beam_free_run(self.step, self.state0, self.B, self.W, T, START, END, **hooks)


def as_recorded(rec):
    """the oracle's own float64 records as a search hands them out: the costs in float32"""
    return dict(rec, cost=rec["cost"].astype(np.float32))


# ====================================================================================================================
# the ban rule and the paths it reads
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


def slot_paths(tok, par, t, G=1):
    """paths (B, W, t + 1) of the slots of fringe t, read along par (an empty slot: zeros); the roots sit in the first slot of each of
    the G groups"""
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
    filled = par[t] >= 0 if t > 0 else np.broadcast_to(np.arange(W) % (W // G) == 0, (B, W))
    return np.where(filled[:, :, None], out, 0)


def ban_mask(paths, vocab, cons, rule=banned_tokens):
    """bool (B * W, V): the ban set of every slot of a fringe"""
    m, g, sup = cons
    B, W, _ = paths.shape
    out = np.zeros((B * W, vocab), bool)
    if rule is banned_tokens and tuple(cons) == NONE:
        return out
    for r, p in enumerate(paths.reshape(B * W, -1).tolist()):
        ids = [v for v in rule(p, m, g, sup) if 0 <= v < vocab]
        out[r, ids] = True
    return out


# ====================================================================================================================
# the walk: a search's records against the oracle, teacher-forced on them
# ====================================================================================================================

def check_records(rec, orc, nll_abs, tag, cons=None, G=1, lam=0.0, alpha_bounds=None, hist=None):
    """The records (tok, cost, par [T+1][B][W], end [T][B][W], what beam.replay_hypotheses reads) of a search of beam width W in G
    groups of W' = W / G slots, diversity penalty `lam`, constraints `cons`, walked by `orc`.  `nll_abs`: the bound of B in nats, or
    (tokens other than <end>, every token).

    A  exact.  The costs are float32; fringe 0 holds <start> at cost 0 in slot g*W' of every group and nothing else; harvest flags and
       done per group, nothing harvested before min_length; par = -1 exactly where cost = +inf; a finished group has no filled slot; a
       parent is a live slot of its child's group; a child costs at least its parent; inside a group the keys fl32(cost + fl32(lam *
       n_v)) ascend, n_v counted from the recorded tokens of the earlier groups at that step; a live group fills min(W', candidates
       that exist) slots (without bans and with V >= W: every slot); no recorded token is banned for its parent; `hist` [B][W][T+1]
       equals the paths along par.
    B  step cost: cost[t + 1][b][w] - cost[t][b][parent] against the oracle's unmasked -log p of that token for that parent, within
       nll_abs plus one fp32 spacing of the cumulative cost -- the recorded cost must not contain the penalty.
    C  selection, per group, within sel = 2 nll_abs (two candidates, each off by at most nll_abs): over the oracle's unbanned
       candidates of the group's live nodes, keyed with lam * n_v, every chosen candidate is at most sel above the W'-th key (where
       W' candidates exist) and every candidate more than sel below it is chosen.
    D  with `alpha_bounds` (max |d alpha|, worst per-row relative L2): the recorded attention map rec["alpha"][t] of every live row
       against the oracle's, non-negative, row sums within ALPHA_SUM of 1.
    B and C leave out no live slot (the excluded share is 0 and is asserted).  Returns the measured worst values; raises
    AssertionError with the first offenders."""
    tok, cost, par, end = rec["tok"], rec["cost"], rec["par"], rec["end"].astype(bool)
    Tn, B, W = end.shape
    cons = NONE if cons is None else cons
    Wg = W // G
    grp = np.arange(W) // Wg
    roots = np.arange(W) % Wg == 0
    nll_word, nll_abs = nll_abs if isinstance(nll_abs, tuple) else (nll_abs, nll_abs)
    m_len, sel = cons[0], 2 * nll_abs
    f32 = np.float32
    assert W % G == 0 and tok.shape == cost.shape == par.shape == (Tn + 1, B, W) and cost.dtype == f32
    assert (tok[0][:, roots] == START).all() and (cost[0][:, roots] == 0).all(), (tag, "every group is seeded in its first slot")
    assert np.isinf(cost[0][:, ~roots]).all() and (tok[0][:, ~roots] == 0).all() and (par[0] == -1).all(), (tag, "fringe 0")
    done = np.zeros((B, G), bool)
    m = dict(nll=0.0, nll_at=None, nll_w=0.0, chosen=-np.inf, missed=-np.inf, a_max=0.0, a_l2=0.0, a_sum=0.0, live=0, checked=0,
             harvested=0)
    bad = []
    for t, logp, alpha in orc.follow(rec):
        logp = logp.double()
        Vn = logp.shape[1]
        k = min(W, Vn)
        c_t = cost[t].astype(np.float64)
        occupied = np.isfinite(c_t)
        ended = occupied & (tok[t] == END) & ~done[:, grp]
        assert np.array_equal(end[t], ended), (tag, t, "harvest flags per group")
        assert not (ended.any() and t <= m_len), (tag, t, "harvested before min_length words")
        m["harvested"] += int(ended.sum())
        live = occupied & ~ended & ~done[:, grp]
        done = done | ~live.reshape(B, G, Wg).any(2)
        live &= ~done[:, grp]
        n_c, n_p, n_t = cost[t + 1], par[t + 1], tok[t + 1]
        filled = n_p >= 0
        assert np.array_equal(filled, np.isfinite(n_c)), (tag, t, "par = -1 exactly where cost = +inf")
        assert not filled[done[:, grp]].any(), (tag, t, "a finished group has a non-empty slot")
        assert (n_p < W).all() and (n_t[~filled] == 0).all(), (tag, t)
        bb, ww = np.nonzero(filled)
        pw = n_p[bb, ww].astype(np.int64)
        assert (pw // Wg == ww // Wg).all(), (tag, t, "a parent lies in its child's group")
        assert live[bb, pw].all(), (tag, t, "the parent of a non-empty slot is a live slot")
        assert (n_c[bb, ww] >= cost[t][bb, pw]).all(), (tag, t, "a child costs at least its parent")
        # n_v of every recorded slot, and the keys of a group in slot order
        earlier = filled[:, None, :] & (grp[None, None, :] < grp[None, :, None])          # (B, slot, earlier slot)
        n_rec = ((n_t[:, :, None] == n_t[:, None, :]) & earlier).sum(2)
        key_rec = np.where(filled, (n_c + (f32(lam) * n_rec.astype(f32)).astype(f32)).astype(f32), f32(np.inf)).reshape(B, G, Wg)
        assert (key_rec[:, :, :-1] <= key_rec[:, :, 1:]).all(), (tag, t, "the keys of a group ascend")
        m["live"] += int(live.sum())
        # (the inputs keep every top-W probability far above the fp32 underflow, where -log p would be +inf: an empty slot)
        ban = ban_mask(slot_paths(tok, par, t, G), Vn, cons)                               # (B * W, V)
        n_cand = np.where(live, np.minimum(k, Vn - ban.reshape(B, W, Vn).sum(2)), 0).reshape(B, G, Wg).sum(2)
        assert np.array_equal(filled.reshape(B, G, Wg).sum(2), np.minimum(Wg, n_cand)), (tag, t, "slots filled")
        if alpha_bounds is not None and live.any():                                        # D
            lr = torch.from_numpy(live.reshape(-1))
            got, ref = torch.from_numpy(rec["alpha"][t]).double()[lr], alpha.double()[lr]
            m["a_max"] = max(m["a_max"], (got - ref).abs().max().item())
            m["a_l2"] = max(m["a_l2"], ((got - ref).norm(dim=1) / ref.norm(dim=1)).max().item())
            m["a_sum"] = max(m["a_sum"], (got.sum(1) - 1).abs().max().item())
            assert (got >= 0).all(), (tag, t, "a negative attention weight")
        if bb.size == 0:
            continue
        assert not ban[bb * W + pw, n_t[bb, ww]].any(), (tag, t, "a recorded token is banned for its parent")
        # B: one number per filled slot per iteration
        rows = torch.from_numpy(bb * W + pw)
        nll_o = -logp[rows, torch.from_numpy(n_t[bb, ww])].numpy()
        nll_g = n_c[bb, ww].astype(np.float64) - c_t[bb, pw]
        err = np.abs(nll_g - nll_o) - np.spacing(n_c[bb, ww]).astype(np.float64)
        m["checked"] += int(bb.size)
        i = int(err.argmax())
        if err[i] > m["nll"]:
            m["nll"], m["nll_at"] = float(err[i]), (t, int(bb[i]), int(ww[i]), int(pw[i]), int(n_t[bb[i], ww[i]]))
        if err[i] > nll_abs:
            bad.append(("B", t, int(bb[i]), int(ww[i]), float(err[i])))
        word = n_t[bb, ww] != END
        if word.any():
            m["nll_w"] = max(m["nll_w"], float(err[word].max()))
            if err[word].max() > nll_word:
                j = int(np.where(word, err, -np.inf).argmax())
                bad.append(("B word", t, int(bb[j]), int(ww[j]), float(err[j])))
        # C: per group, the oracle's unbanned candidates of the group's live nodes with their penalties; a node's k best suffice
        masked = logp.masked_fill(torch.from_numpy(ban), -np.inf) if ban.any() else logp
        tv, ti = torch.topk(masked, k, dim=1)
        tv, ti = tv.view(B, W, k).numpy(), ti.view(B, W, k).numpy()
        n_o = ((ti[:, :, :, None] == n_t[:, None, None, :]) & earlier[:, :, None, :]).sum(3)      # (B, W, k)
        cand = np.where(live[:, :, None], c_t[:, :, None] - tv + lam * n_o, np.inf)
        kth = np.partition(cand.reshape(B, G, Wg * k), Wg - 1, axis=2)[:, :, Wg - 1]              # (B, G); +inf: fewer than W' exist
        over = (c_t[bb, pw] + nll_o + lam * n_rec[bb, ww]) - kth[bb, ww // Wg]
        over = np.where(np.isfinite(kth[bb, ww // Wg]), over, -np.inf)                            # fewer than W' candidates: all are chosen
        m["chosen"] = max(m["chosen"], float(over.max()))
        ident = np.arange(W)[None, :, None] * Vn + ti
        chosen = np.where(filled, n_p.astype(np.int64) * Vn + n_t, -1)
        present = (ident[:, :, :, None] == chosen[:, None, None, :]).any(3)
        kth_w = np.where(np.isfinite(kth), kth, np.inf)[:, grp]
        with np.errstate(invalid="ignore"):
            below = np.where(present | ~np.isfinite(cand), -np.inf, kth_w[:, :, None] - cand)     # not chosen: how far below the W'-th
        m["missed"] = max(m["missed"], float(below.max()))
        if over.max() > sel or below.max() > sel:
            bad.append(("C", t, int(bb[int(over.argmax())]), float(over.max()), float(below.max())))
    if hist is not None:
        assert np.array_equal(hist.astype(np.int64), slot_paths(tok, par, Tn, G)), (tag, "the kept paths are not the paths along par")
    excluded = 1.0 - m["checked"] / max(1, int((par[1:] >= 0).sum()))
    print(f"MEASURE {tag}: |d nll| of words {m['nll_w']:.2e}, of all tokens {m['nll']:.2e} nats at (t, b, w, parent, token) "
          f"{m['nll_at']}; selection: chosen above the W'-th key {m['chosen']:.2e}, missed below it {m['missed']:.2e}; live slots "
          f"{m['live']}, live share {m['live'] / float(Tn * B * W):.2f}, harvested {m['harvested']}, slots checked {m['checked']}, "
          f"excluded share {excluded}"
          + (f"; alpha max {m['a_max']:.2e} rel_l2 {m['a_l2']:.2e} |sum - 1| {m['a_sum']:.2e}" if alpha_bounds else ""))
    assert excluded == 0.0
    assert not bad, (tag, nll_abs, bad[:8])
    assert m["nll_w"] <= nll_word and m["nll"] <= nll_abs and m["chosen"] <= sel and m["missed"] <= sel, (tag, m)
    if alpha_bounds:
        assert m["a_max"] <= alpha_bounds[0] and m["a_l2"] <= alpha_bounds[1] and m["a_sum"] <= ALPHA_SUM, (tag, m)
    return m


def beam_distance(a, b, rec):
    """max |d nll| of the recorded children (every token, words) and, for attention decoders, the alpha distances over the live rows
    (relative to b's) between two oracles walking the same records: the quantities checks B and D bound.  With fp32 and float64
    arithmetic of the same restatement, teacher-forced on the float64 oracle's own free run, this is the floor of any implementation
    that accumulates in fp32."""
    out = dict(nll=0.0, nll_word=0.0, a_max=0.0, a_l2=0.0)
    B, W = rec["tok"].shape[1:]
    done = np.zeros(B, bool)
    for (t, lpa, ala), (_, lpb, alb) in zip(a.follow(rec), b.follow(rec)):
        live = np.isfinite(rec["cost"][t]) & ~rec["end"][t].astype(bool) & ~done[:, None]
        done = done | ~live.any(1)
        live &= ~done[:, None]
        bb, ww = np.nonzero(rec["par"][t + 1] >= 0)
        if bb.size:
            rows = torch.from_numpy(bb * W + rec["par"][t + 1][bb, ww])
            col = torch.from_numpy(rec["tok"][t + 1][bb, ww])
            d = (lpa[rows, col].double() - lpb[rows, col].double()).abs()
            out["nll"] = max(out["nll"], d.max().item())
            if (col != END).any():
                out["nll_word"] = max(out["nll_word"], d[col != END].max().item())
        if ala is not None and live.any():
            lr = torch.from_numpy(live.reshape(-1))
            d = ala.double()[lr] - alb.double()[lr]
            out["a_max"] = max(out["a_max"], d.abs().max().item())
            out["a_l2"] = max(out["a_l2"], (d.norm(dim=1) / alb.double()[lr].norm(dim=1)).max().item())
    return out
