"""Beam decoding on MI355X.

Two different things exist in the reference and both are mirrored:

* ``quirky_beam``  -- the live path of ``rnn.py:60-108`` (``sentence_index(beam_size>0)``, bs=1): one
  recurrent state threaded through every beam, candidates ranked by the current-step raw logit only.
* ``beam_search``  -- the textbook search of ``beam_search.py:45-97`` (cumulative -log p, <end> moves a
  node to the hypotheses, stable sort by cost), batched over images: every step is ONE set of device
  launches over the nodes of all images (st_embedding_rows, st_gather_state, st_rnn_step, st_softmax_topk and,
  by default, st_beam_select for the fringe selection, so that a search needs one host round trip in all).
  The reference's list bookkeeping (``Node`` parents, stable ``sorted``) is reproduced literally, including its
  float32 cost accumulation under NumPy 2 and the fact that nodes ending on the last iteration are never
  harvested; ``beam_search_host`` keeps that bookkeeping on the host per iteration (the cross-check).

Constrained search (``min_length``, ``no_repeat_ngram_size``, ``suppress_tokens``, ``length_penalty``): a successor v of a node
with the path s_0 .. s_t (s_0 = <start>) is BANNED iff v is suppressed, or v is <end> and t < min_length, or appending v would
repeat an n-gram of size g already on the path.  Bans act before a row is cut to its k successors (st_beam_ban_topk takes the
k most probable unbanned entries) and leave the probabilities alone: a cost stays the model's own -log p.  Every node inherits
its parent's path inside the selection kernel (st_beam_select with its path buffers), so a constrained iteration has the
launches of an unconstrained one.  ``length_penalty`` a only re-ranks the harvested hypotheses, by cost / n**a.

Diverse (group) beam search (Vijayakumar et al., AAAI 2018; ``num_beam_groups`` = G, ``diversity_penalty`` = lambda): the W slots
are G groups of W' = W / G, group g = slots g*W' .. (g+1)*W' - 1, each a search of its own (its own root in slot g*W', harvest
flags, done flag and hypotheses; a parent lies in its child's group).  Every iteration runs the model step and the top-k launch on
all B*W rows as before; the selection (st_beam_select, one launch) handles the groups of an image in the order 0 .. G-1 and
ranks a candidate (node w, word v) of group g by key = fl32(raw + fl32(lambda * n_v)), raw = fl32(cost[w] + fl32(-log p)), n_v = the
number of occupied slots of the new fringes of groups 0 .. g-1, chosen in this same iteration, that hold v (a count, <end>
included).  The recorded cost is raw: the penalty decides the selection of the current step only and is never carried, which is
the paper's objective (cumulative log-probability plus a current-step diversity term), so a cost stays the model's own -log p.
HuggingFace lets the penalty accumulate in the beam score; that is deliberately NOT followed here.  k = min(W, V) list entries per
node suffice: a node of group g is penalised on at most g*W' <= W - W' distinct words, so at least W' of its k most probable
(unbanned) words carry no penalty, and every word outside the list has a raw cost, hence a key, no smaller than theirs.
"""
import ctypes as C
import operator

import numpy as np
import torch

from ._lib import check, dtype_code as _dtc, lib
from ._lib import ptr as _cp, stream as _stream
from .rnn import CAP_MAX, up8

# include/showtell_hip.h
ST_BEAM_MAX_NGRAM, ST_BEAM_MAX_SUPPRESS, ST_BEAM_MAX_HIST, ST_BEAM_MAX_VOCAB = 16, 64, 64, 524288


class BeamConstraints:
    """The validated constraints of one search; ``active`` says whether the search is a constrained one at all (any of the three
    set: an empty ``suppress_tokens`` list counts).  ``keep_paths``: the search carries every node's path (needed for n-gram
    blocking, kept whenever an active search fits it).  ``bans``: there is something to ban, so the top-k launch is
    st_beam_ban_topk; ``suppress_tokens=[]`` is active and keeps its paths, but bans nothing and runs st_softmax_topk (the same
    bits)."""

    def __init__(self, vocab_size, max_length, min_length=0, no_repeat_ngram_size=0, suppress_tokens=None, length_penalty=0.0):
        m, g = int(min_length), int(no_repeat_ngram_size)
        if m != min_length or g != no_repeat_ngram_size:
            raise ValueError(f"min_length and no_repeat_ngram_size must be integers (got {min_length}, {no_repeat_ngram_size})")
        if m < 0:
            raise ValueError(f"min_length must be >= 0 (got {m})")
        if not 0 <= g <= ST_BEAM_MAX_NGRAM:
            raise ValueError(f"no_repeat_ngram_size must be 0..{ST_BEAM_MAX_NGRAM} (got {g})")
        sup = None if suppress_tokens is None else [int(v) for v in suppress_tokens]
        if sup is not None:
            if len(sup) > ST_BEAM_MAX_SUPPRESS:
                raise ValueError(f"at most {ST_BEAM_MAX_SUPPRESS} suppress_tokens (got {len(sup)})")
            bad = [v for v in sup if not 0 <= v < vocab_size]
            if bad:
                raise ValueError(f"suppress_tokens outside [0, {vocab_size}): {bad}")
        if g > 0 and max_length + 1 > ST_BEAM_MAX_HIST:
            raise ValueError(f"no_repeat_ngram_size needs max_length + 1 <= {ST_BEAM_MAX_HIST} (got max_length={max_length})")
        a = float(length_penalty)
        if a != a:
            raise ValueError("length_penalty is NaN")
        self.min_length, self.ngram, self.suppress, self.length_penalty = m, g, sup, a
        self.active = m > 0 or g > 0 or sup is not None
        if self.active and vocab_size > ST_BEAM_MAX_VOCAB:
            raise ValueError(f"constrained beam search needs a vocabulary of at most {ST_BEAM_MAX_VOCAB} entries (got {vocab_size})")
        self.keep_paths = self.active and max_length + 1 <= ST_BEAM_MAX_HIST
        self.bans = m > 0 or g > 0 or bool(sup)

    def suppress_on(self, device):
        """(device tensor or None, count): the suppress list as st_beam_ban_topk takes it, uploaded once per search."""
        if not self.suppress:
            return None, 0
        return torch.tensor(self.suppress, dtype=torch.long, device=device), len(self.suppress)


DIVERSE_ON_DEVICE_ONLY = "diverse beam search (num_beam_groups > 1) runs on the device only: on_device and beam_width * min(beam_width, V) <= 64"


def check_groups(beam_width, vocab_size, num_beam_groups=1, diversity_penalty=0.0, on_device=True):
    """(G, lambda) of a diverse search, validated before the device is touched: G an integer in 1..W that divides W, lambda >= 0
    (and 0 with one group: there is nothing to differ from); G > 1 runs on the device only, so it needs W * min(W, V) <= 64."""
    W = int(beam_width)
    try:
        G = None if isinstance(num_beam_groups, bool) else operator.index(num_beam_groups)      # an integer type: 2.0 is none
    except TypeError:
        G = None
    if G is None or not 1 <= G <= W:
        raise ValueError(f"num_beam_groups must be an integer in 1..beam_width={W} (got {num_beam_groups!r})")
    if W % G:
        raise ValueError(f"beam_width={W} is not a multiple of num_beam_groups={G}")
    lam = float(diversity_penalty)
    if not 0.0 <= lam < float("inf"):
        raise ValueError(f"diversity_penalty must be finite and >= 0 (got {diversity_penalty})")
    if G == 1 and lam != 0.0:
        raise ValueError(f"diversity_penalty={lam} needs num_beam_groups > 1")
    if G > 1 and (not on_device or W * min(W, int(vocab_size)) > 64):
        raise ValueError(DIVERSE_ON_DEVICE_ONLY)
    return G, lam


def group_records(rec, g, num_beam_groups):
    """Group g of the records of a diverse search as records of a search W' = W / G wide: tok / cost / par / end (and hist, alpha)
    cut to the group's slots, `par` rebased to the group, so that ``replay_hypotheses`` serves a group unchanged."""
    G = int(num_beam_groups)
    W = rec["tok"].shape[2]
    if G < 1 or W % G or not 0 <= g < G:
        raise ValueError(f"group {g} of {G} over {W} slots")
    Wg = W // G
    sl = slice(g * Wg, (g + 1) * Wg)
    par = rec["par"][:, :, sl]
    out = dict(tok=rec["tok"][:, :, sl], cost=rec["cost"][:, :, sl], par=np.where(par >= 0, par - g * Wg, -1).astype(rec["par"].dtype),
               end=rec["end"][:, :, sl])
    if "hist" in rec:
        out["hist"] = rec["hist"][:, sl]
    if "alpha" in rec:
        a = rec["alpha"]
        B = rec["tok"].shape[1]
        out["alpha"] = np.ascontiguousarray(a.reshape(a.shape[0], B, W, a.shape[2])[:, :, sl]).reshape(a.shape[0], B * Wg, a.shape[2])
    return out


def replay_groups(rec, num_beam_groups, num_hypotheses, length_penalty=0.0):
    """Per image a list of G lists: ``replay_hypotheses`` of every sliced group (harvested and ranked on its own)."""
    per = []
    for g in range(num_beam_groups):
        r = group_records(rec, g, num_beam_groups)
        per.append(replay_hypotheses(r["tok"], r["cost"], r["par"], r["end"], num_hypotheses, r.get("alpha"), length_penalty))
    return [[per[g][b] for g in range(num_beam_groups)] for b in range(rec["tok"].shape[1])]


class _Stepper:
    """Device-side single-step decoder over n rows with explicit state tensors [L][n][H]."""

    def __init__(self, rnn):
        self.rnn = rnn
        self.prm, self.keep = rnn._c_params()
        self.dt = rnn.compute_dtype
        self.dev = rnn.linear.weight.device
        self.L, self.H, self.E, self.V = rnn.num_layers, rnn.hidden, rnn.embed_dim, rnn.vocab_size
        self.Vp = up8(self.V)
        self.lstm = rnn.cell != "gru"

    def embed(self, ids):
        ids = torch.as_tensor(ids, dtype=torch.long, device=self.dev).contiguous()
        x = torch.empty(ids.numel(), self.E, device=self.dev, dtype=self.dt)
        check(lib().st_embedding_rows(_cp(self.keep[0]), _cp(ids), _cp(x), ids.numel(), self.E, self.V, self.E, _dtc(self.dt), _stream()),
              "st_embedding_rows")
        return x

    def gather(self, state, idx):
        idx = torch.as_tensor(idx, dtype=torch.int32, device=self.dev).contiguous()
        out = []
        for s in state:
            d = torch.empty(self.L, idx.numel(), self.H, device=self.dev, dtype=self.dt)
            check(lib().st_gather_state(_cp(s), _cp(idx), _cp(d), self.L, s.shape[1], idx.numel(), self.H, _dtc(self.dt), _stream()),
                  "st_gather_state")
            out.append(d)
        return tuple(out)

    def step(self, x, state, want_logits=True):
        n = x.shape[0]
        h_out = torch.empty(self.L, n, self.H, device=self.dev, dtype=self.dt)
        c_out = torch.empty_like(h_out) if self.lstm else None
        logits = torch.empty(n, self.Vp, device=self.dev, dtype=torch.float32) if want_logits else None
        h_in = state[0] if state is not None else None
        c_in = state[1] if (state is not None and self.lstm) else None
        check(lib().st_rnn_step(C.byref(self.prm), _cp(x), n, _cp(h_in), _cp(c_in), _cp(h_out), _cp(c_out), _cp(logits), self.Vp,
                                _stream()), "st_rnn_step")
        return logits, ((h_out, c_out) if self.lstm else (h_out,))

    def topk(self, logits, k, raw):
        n = logits.shape[0]
        p = torch.empty(n, k, device=self.dev, dtype=torch.float32)
        i = torch.empty(n, k, device=self.dev, dtype=torch.long)
        check(lib().st_softmax_topk(_cp(logits), self.Vp, n, self.V, k, _cp(p), _cp(i), int(raw), _stream()), "st_softmax_topk")
        return p.cpu().numpy(), i.cpu().numpy()

    def ban_topk(self, logits, k, hist, hist_len, ngram, suppress, n_suppress, end_id, ban_end):
        """topk(raw=False) over the entries outside each row's ban set; hist (n, ld) int32 on the device holds the rows' paths."""
        n = logits.shape[0]
        p = torch.empty(n, k, device=self.dev, dtype=torch.float32)
        i = torch.empty(n, k, device=self.dev, dtype=torch.long)
        check(lib().st_beam_ban_topk(_cp(logits), self.Vp, n, self.V, k, _cp(hist), hist.shape[1] if hist is not None else 0, hist_len,
                                     ngram, _cp(suppress), n_suppress, end_id, int(ban_end), _cp(p), _cp(i), _stream()), "st_beam_ban_topk")
        return p.cpu().numpy(), i.cpu().numpy()


def _feat(rnn, cnn_feature):
    return rnn._feature(cnn_feature)


def quirky_beam(rnn, cnn_feature, beam_size, steps=CAP_MAX):
    """rnn.py:60-108, bs=1 only (main.py:81-82 forces batch_size=1 when --beam_size>0)."""
    if cnn_feature.shape[0] != 1:
        raise ValueError("beam_size > 0 only works with batch_size=1 (rnn.py:60)")
    with torch.no_grad():
        st = _Stepper(rnn)
        logits, state = st.step(_feat(rnn, cnn_feature), None)                     # rnn.py:61-62
        _, ti = st.topk(logits, beam_size, raw=True)                               # rnn.py:63
        old_word = [int(w) for w in ti[0]]
        old_sent = [[w] for w in old_word]
        idx = 1
        while idx < steps:                                                         # rnn.py:78
            idx += 1
            new_sent, new_word, new_prob = [], [], []
            for k in range(beam_size):
                logits, state = st.step(st.embed([old_word[k]]), state)            # rnn.py:85-88: ONE shared state
                tv, ti = st.topk(logits, beam_size, raw=True)                      # rnn.py:90-91
                for j in range(beam_size):
                    new_sent.append(old_sent[k] + [int(ti[0, j])])
                    new_word.append(int(ti[0, j]))
                    new_prob.append(float(tv[0, j]))
            old_sent = [x for _, x in sorted(zip(new_prob, new_sent), reverse=True)][:beam_size]   # rnn.py:102
            old_word = [x for _, x in sorted(zip(new_prob, new_word), reverse=True)][:beam_size]   # rnn.py:103
        return torch.tensor(old_sent[0], dtype=torch.long, device=cnn_feature.device)   # rnn.py:106-108


def beam_search(rnn, cnn_feature, beam_width=4, num_hypotheses=1, max_length=50, start_id=1, end_id=2, on_device=True,
                min_length=0, no_repeat_ngram_size=0, suppress_tokens=None, length_penalty=0.0, num_beam_groups=1, diversity_penalty=0.0):
    """beam_search.py:45-97 for every image of the batch; see ``beam_search_host`` for the contract.  With ``on_device`` (and
    beam_width**2 <= 64) the fringe selection of every iteration also runs on the GPU (``st_beam_select``) over fixed
    (image, slot) rows, so the whole search needs ONE host round trip instead of three per iteration; the Node bookkeeping
    (harvest order, stable sort of the hypotheses, parent back-tracking) is replayed on the host from the recorded fringes.
    The only arithmetic that differs from the host path is -log p: a correctly rounded float32 logarithm on the device, NumPy's
    float32 log on the host (<= 1 ulp apart; the golden sequences are reproduced by both).

    Constraints (module docstring): ``min_length`` words before <end>, ``no_repeat_ngram_size``, ``suppress_tokens`` (ids that never
    appear) act inside the device loop; ``length_penalty`` a ranks the harvested hypotheses by cost / n**a (n tokens after <start>,
    <end> included) and returns the raw cost.  With all four at their defaults the call is the launch sequence it was.

    Diverse beam search (module docstring): ``num_beam_groups`` = G > 1 splits the beam into G groups of beam_width / G slots and
    ``diversity_penalty`` = lambda >= 0 charges a group's candidates lambda per earlier group's slot that took the same word at
    this step; the penalty is never recorded in a cost (the paper's objective, not HuggingFace's accumulating score).  The
    return value is then, per image, a list of G lists of at most `num_hypotheses` (tokens, cost) pairs, each group harvested and
    ranked on its own.  Device only.  With G = 1 the return value and the launch sequence are what they were."""
    G, lam = check_groups(beam_width, rnn.vocab_size, num_beam_groups, diversity_penalty, on_device)
    k = min(beam_width, rnn.vocab_size)
    cons = dict(min_length=min_length, no_repeat_ngram_size=no_repeat_ngram_size, suppress_tokens=suppress_tokens)
    if G > 1:
        BeamConstraints(rnn.vocab_size, max_length, length_penalty=length_penalty, **cons)
        r = beam_search_records(rnn, cnn_feature, beam_width, max_length, start_id, end_id, num_beam_groups=G, diversity_penalty=lam, **cons)
        return replay_groups(r, G, num_hypotheses, float(length_penalty))
    if not on_device or beam_width * k > 64:
        return beam_search_host(rnn, cnn_feature, beam_width, num_hypotheses, max_length, start_id, end_id, length_penalty=length_penalty,
                                **cons)
    BeamConstraints(rnn.vocab_size, max_length, length_penalty=length_penalty, **cons)      # (length_penalty checked before the search)
    r = beam_search_records(rnn, cnn_feature, beam_width, max_length, start_id, end_id, **cons)
    return replay_hypotheses(r["tok"], r["cost"], r["par"], r["end"], num_hypotheses, length_penalty=length_penalty)


def beam_search_records(rnn, cnn_feature, beam_width=4, max_length=50, start_id=1, end_id=2, min_length=0, no_repeat_ngram_size=0,
                        suppress_tokens=None, num_beam_groups=1, diversity_penalty=0.0):
    """The device loop of ``beam_search`` on its own: every iteration's fringe over fixed (image, slot) rows, as numpy arrays
    dict(tok, cost, par [max_length+1][B][W], end [max_length][B][W]) -- what ``replay_hypotheses`` reads.  Needs
    beam_width * min(beam_width, V) <= 64 (st_beam_select).  With something to ban the top-k launch is st_beam_ban_topk; a
    constrained search hands st_beam_select its path buffers, and the records gain hist [B][W][max_length+1] int32: the path of
    every slot of the last fringe, as the search itself kept it.  With ``num_beam_groups`` = G > 1 the layout stays, slots
    g*W/G .. (g+1)*W/G - 1 are group g (``group_records`` cuts one out), `par` holds image-wide slot indices."""
    G, lam = check_groups(beam_width, rnn.vocab_size, num_beam_groups, diversity_penalty)
    k = min(beam_width, rnn.vocab_size)
    bc = BeamConstraints(rnn.vocab_size, max_length, min_length, no_repeat_ngram_size, suppress_tokens)
    with torch.no_grad():
        st = _Stepper(rnn)
        dev = st.dev
        B, W = cnn_feature.shape[0], beam_width
        n = B * W
        _, state = st.step(_feat(rnn, cnn_feature), None, want_logits=False)      # state after the image-feature step (rnn.py:41,49)
        state = st.gather(state, torch.arange(B, device=dev, dtype=torch.int32).repeat_interleave(W))   # slot (b, w) <- image b
        tok = torch.zeros(B, W, device=dev, dtype=torch.long); tok[:, ::W // G] = start_id    # beam_search.py:66, once per group
        cost = torch.full((B, W), float("inf"), device=dev, dtype=torch.float32); cost[:, ::W // G] = 0.0
        done = torch.zeros(B * G, device=dev, dtype=torch.uint8)
        rec_tok = torch.zeros(max_length + 1, B, W, device=dev, dtype=torch.long)
        rec_cost = torch.full((max_length + 1, B, W), float("inf"), device=dev, dtype=torch.float32)
        rec_par = torch.full((max_length + 1, B, W), -1, device=dev, dtype=torch.int32)
        rec_end = torch.zeros(max_length, B, W, device=dev, dtype=torch.uint8)
        rec_tok[0], rec_cost[0] = tok, cost
        gidx = torch.empty(n, device=dev, dtype=torch.int32)
        tp = torch.empty(n, k, device=dev, dtype=torch.float32)
        ti = torch.empty(n, k, device=dev, dtype=torch.long)
        hist, hp, ld = None, (None, None), 0
        sup, n_sup = bc.suppress_on(dev)
        if bc.keep_paths:                                                             # two buffers: a fringe reads one, writes the other
            ld = max_length + 1
            hist = torch.zeros(2, n, ld, device=dev, dtype=torch.int32); hist[0, :, 0] = start_id
            hp = (_cp(hist[0]), _cp(hist[1]))
        for t in range(max_length):                                                   # beam_search.py:69
            x = st.embed(tok.view(-1))
            logits, new_state = st.step(x, state)
            ntok, ncost = rec_tok[t + 1], rec_cost[t + 1]
            if not bc.bans:
                check(lib().st_softmax_topk(_cp(logits), st.Vp, n, st.V, k, _cp(tp), _cp(ti), 0, _stream()), "st_softmax_topk")
            else:                                                                     # the path of a fringe-t node has t + 1 tokens
                check(lib().st_beam_ban_topk(_cp(logits), st.Vp, n, st.V, k, hp[t & 1], ld, t + 1, bc.ngram, _cp(sup), n_sup, end_id,
                                             int(t < bc.min_length), _cp(tp), _cp(ti), _stream()), "st_beam_ban_topk")
            check(lib().st_beam_select(_cp(tok), _cp(cost), _cp(done), _cp(tp), _cp(ti), B, W, G, k, end_id, lam, _cp(ntok), _cp(ncost),
                                       _cp(rec_par[t + 1]), _cp(rec_end[t]), _cp(gidx), hp[t & 1], hp[(t + 1) & 1], ld, t + 1, _stream()),
                  "st_beam_select")
            state = st.gather(new_state, gidx)
            tok, cost = ntok, ncost
        rec = dict(tok=rec_tok.cpu().numpy(), cost=rec_cost.cpu().numpy(), par=rec_par.cpu().numpy(), end=rec_end.cpu().numpy())
        if hist is not None:
            rec["hist"] = hist[max_length & 1].view(B, W, ld).cpu().numpy()
        return rec


def _ranked(hyp, num_hypotheses, length_penalty):
    """The first `num_hypotheses` of harvested (iteration, slot, cost) triples: a stable sort by cost (beam_search.py:96) or, with
    length_penalty a != 0, by cost / n**a in float64, n = the harvest iteration = the tokens after <start>, <end> included."""
    if length_penalty == 0.0:
        return sorted(hyp, key=lambda e: e[2])[:num_hypotheses]
    return sorted(hyp, key=lambda e: float(e[2]) / float(max(e[0], 1)) ** length_penalty)[:num_hypotheses]


def replay_hypotheses(h_tok, h_cost, h_par, h_end, num_hypotheses, alphas=None, length_penalty=0.0):
    """The Node bookkeeping of beam_search.py:69-97, replayed on the host from the records of a device search over fixed
    (image, slot) rows: h_tok / h_cost / h_par [max_length+1][B][W] (fringe after each iteration, parent slots),
    h_end [max_length][B][W] (harvest flags).  Returns, per image, at most `num_hypotheses` (tokens, cost) pairs.

    With `alphas` ([max_length][B*W][P], the attention map of every row at every iteration) each pair becomes
    (tokens, cost, extras), extras a float32 tensor (len(tokens) - 1, P): the extras of a node are the alpha computed while
    producing it, i.e. that of its PARENT's row one iteration earlier, alphas[t-1][b*W + parent slot] for node (t, w).

    `length_penalty` a ranks the hypotheses by cost / n**a instead (n = tokens after <start>, <end> included; float64 quotient of
    the recorded float32 cost, stable); the returned cost stays the raw one."""
    length_penalty = float(length_penalty)
    B, W = h_tok.shape[1], h_tok.shape[2]
    out = []
    eb, et, ew = np.nonzero(np.transpose(h_end, (1, 0, 2)))                           # one pass over the flags: image-major
    first = np.searchsorted(eb, np.arange(B + 1))
    for b in range(B):
        if first[b] == first[b + 1]:                                                  # nothing ended in time
            out.append([])
            continue
        hyp = []                                                                      # (iteration of the node, slot, cost) in harvest order
        for t, w in zip(et[first[b]:first[b + 1]], ew[first[b]:first[b + 1]]):        # iteration-major, slot order inside (beam_search.py:72-76)
            hyp.append((int(t), int(w), h_cost[t, b, w]))
        res = []
        for t, w, c in _ranked(hyp, num_hypotheses, length_penalty):                  # beam_search.py:96 (stable)
            seq, ext = [], []
            while t >= 0 and w >= 0:
                seq.append(int(h_tok[t, b, w]))
                if t > 0:
                    par = int(h_par[t, b, w])
                    if alphas is not None:
                        ext.append(alphas[t - 1, b * W + par])
                    w = par
                else:
                    w = -1
                t -= 1
            if alphas is None:
                res.append((seq[::-1], float(c)))
            else:
                ex = np.stack(ext[::-1]) if ext else np.zeros((0, alphas.shape[2]), dtype=np.float32)
                res.append((seq[::-1], float(c), torch.from_numpy(np.ascontiguousarray(ex, dtype=np.float32))))
        out.append(res)
    return out


def beam_search_host(rnn, cnn_feature, beam_width=4, num_hypotheses=1, max_length=50, start_id=1, end_id=2, min_length=0,
                     no_repeat_ngram_size=0, suppress_tokens=None, length_penalty=0.0, num_beam_groups=1, diversity_penalty=0.0):
    """beam_search.py:45-97 for every image of the batch.  Returns, per image, a list of at most
    `num_hypotheses` (token_sequence, cum_cost) pairs; the list is empty when no beam ever emitted
    `end_id` in time (the reference returns [] then).

    Bookkeeping is vectorised over the batch (fixed (B, W, k) candidate blocks; the reference's per-image lists of
    Node objects were 95 % of the time at 256 images) and reproduces the reference's order exactly: candidates are
    laid out node-major in fringe order, each node's k successors in ASCENDING probability (argsort(p)[-k:]), and cut
    with a STABLE sort on the float32 cumulative cost; finished nodes are harvested at the start of an iteration (so
    nodes that end on the last iteration are never harvested), hypotheses are stably sorted by cost at the end.

    Under constraints every fringe node carries its path (`path`, beside the Node table) and its successors come from
    st_beam_ban_topk; the hypotheses are ranked as ``replay_hypotheses`` ranks them.  Diverse search (num_beam_groups > 1) runs
    on the device only and is refused here."""
    check_groups(beam_width, rnn.vocab_size, num_beam_groups, diversity_penalty, on_device=False)
    bc = BeamConstraints(rnn.vocab_size, max_length, min_length, no_repeat_ngram_size, suppress_tokens, length_penalty)
    with torch.no_grad():
        st = _Stepper(rnn)
        B = cnn_feature.shape[0]
        W = beam_width
        k = min(beam_width, st.V)
        _, state = st.step(_feat(rnn, cnn_feature), None, want_logits=False)      # state after the image-feature step (rnn.py:41,49)
        # global node table (parent pointers) for the final back-tracking
        node_parent = [np.full(B, -1, dtype=np.int64)]
        node_value = [np.full(B, start_id, dtype=np.int64)]
        n_nodes = B
        tok = np.full((B, W), -1, dtype=np.int64); tok[:, 0] = start_id              # beam_search.py:66
        cost = np.full((B, W), np.inf, dtype=np.float32); cost[:, 0] = 0.0
        row = np.zeros((B, W), dtype=np.int64); row[:, 0] = np.arange(B)             # row of the node's state
        nid = np.full((B, W), -1, dtype=np.int64); nid[:, 0] = np.arange(B)
        valid = np.zeros((B, W), dtype=bool); valid[:, 0] = True
        done = np.zeros(B, dtype=bool)
        hyp_nodes = [[] for _ in range(B)]                                            # (harvest iteration, node id, cost) in harvest order
        path = None
        if bc.active:
            sup, n_sup = bc.suppress_on(st.dev)
            if bc.keep_paths:
                path = np.zeros((B, W, max_length + 1), dtype=np.int32); path[:, :, 0] = start_id
        for t in range(max_length):                                                   # beam_search.py:69
            ended = valid & (tok == end_id) & ~done[:, None]                          # beam_search.py:72-76
            if ended.any():
                for b, w in zip(*np.nonzero(ended)):
                    hyp_nodes[b].append((t, int(nid[b, w]), cost[b, w]))
            live = valid & ~ended & ~done[:, None]
            done |= ~live.any(axis=1)                                                 # beam_search.py:78-79 (break)
            live &= ~done[:, None]
            lb, lw = np.nonzero(live)                                                 # image-major, fringe order inside an image
            if lb.size == 0:
                break
            x = st.embed(tok[lb, lw])
            logits, new_state = st.step(x, st.gather(state, row[lb, lw]))
            if not bc.active:
                tp, ti = st.topk(logits, k, raw=False)                                # descending; argsort(p)[-k:] is ascending
            else:
                hist = torch.from_numpy(np.ascontiguousarray(path[lb, lw])).to(st.dev) if path is not None else None
                tp, ti = st.ban_topk(logits, k, hist, t + 1, bc.ngram, sup, n_sup, end_id, t < bc.min_length)
            with np.errstate(divide="ignore"):                                        # (a missing successor, p = 0, costs +inf)
                nll = -np.log(tp[:, ::-1].astype(np.float32))                         # beam_search.py:87-92
            cand_cost = np.full((B, W, k), np.inf, dtype=np.float32)
            cand_tok = np.zeros((B, W, k), dtype=np.int64)
            cand_row = np.zeros((B, W, k), dtype=np.int64)
            cand_par = np.zeros((B, W, k), dtype=np.int64)
            cand_cost[lb, lw] = cost[lb, lw][:, None] + nll                           # float32 + float32 (NEP 50: the root's 0.0 is weak)
            cand_tok[lb, lw] = ti[:, ::-1]
            cand_row[lb, lw] = np.arange(lb.size)[:, None]
            cand_par[lb, lw] = nid[lb, lw][:, None]
            cand_slot = np.broadcast_to(np.arange(W)[None, :, None], (B, W, k))
            flat = cand_cost.reshape(B, W * k)
            order = np.argsort(flat, axis=1, kind="stable")[:, :W]                    # beam_search.py:94 (stable sorted()[:beam_width])
            take = np.take_along_axis
            new_cost = take(flat, order, 1)
            valid = np.isfinite(new_cost) & ~done[:, None]
            tok = take(cand_tok.reshape(B, W * k), order, 1)
            row = take(cand_row.reshape(B, W * k), order, 1)
            par = take(cand_par.reshape(B, W * k), order, 1)
            if path is not None:                                                      # a child's path = its parent's + its token
                path = take(path, take(cand_slot.reshape(B, W * k), order, 1)[:, :, None], 1)
                path[:, :, t + 1] = tok
            cost = np.where(valid, new_cost, np.float32(np.inf)).astype(np.float32)
            # register the new nodes
            vb, vw = np.nonzero(valid)
            nid = np.full((B, W), -1, dtype=np.int64)
            nid[vb, vw] = n_nodes + np.arange(vb.size)
            node_parent.append(par[vb, vw]); node_value.append(tok[vb, vw])
            n_nodes += vb.size
            state = new_state
        parent = np.concatenate(node_parent); value = np.concatenate(node_value)
        out = []
        for b in range(B):
            hy = _ranked(hyp_nodes[b], num_hypotheses, bc.length_penalty)             # beam_search.py:96 (stable)
            res = []
            for _, node, c in hy:
                seq = []
                while node >= 0:
                    seq.append(int(value[node])); node = int(parent[node])
                res.append((seq[::-1], float(c)))
            out.append(res)
        return out
