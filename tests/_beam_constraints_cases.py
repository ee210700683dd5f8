"""Shared by test_beam_constraints_inputs.py (CPU) and test_gpu_beam_constraints.py: the decoders and images of the cases, the ban
rule by brute force, and the float64 oracle's own constrained search with its seeded faults.  The rule itself (`banned_tokens`,
written from the three rules of beam.py's docstring, not from the kernel), the paths it reads and the walk of a search's records
are tests/_beam_oracle.py's.
"""
import numpy as np
import torch

from oracle import restatement as R
from tests._beam_oracle import END, START, StepOracle, ban_mask, banned_tokens, beam_distance, slot_paths  # noqa: F401
from tests._util import _bf16

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


# ====================================================================================================================
# decoders, images, the float64 oracle's own constrained search
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


def free_run(orc, cons, Tn=T, rule=banned_tokens, after_cut=False, renormalise=False, own_slot_paths=False):
    """R.beam_free_run under constraints: a node's successors are its W most probable UNBANNED entries at the model's own
    log p.  `rule`, `after_cut` (bans applied to the unconstrained top W), `renormalise` (log p over the unbanned set) and
    `own_slot_paths` (slot w extends the path slot w had, not its parent's) are the seeded faults of test_beam_constraints_inputs.
    Returns the records, with `top_banned` [T][B][W] (at least one of the unconstrained top W is banned), `mass_banned` [T][B][W]
    (probability mass of the ban set) and `live` [T][B][W] of every slot, and `gap` [T][B], the cost distance between the last
    candidate taken into the fringe and the first one left out."""
    B, W, Vn = orc.B, orc.W, orc.V
    k = min(W, Vn)
    top_banned, mass_banned = np.zeros((Tn, B, W), bool), np.zeros((Tn, B, W))
    live_rec = np.zeros((Tn, B, W), bool)
    gap = np.full((Tn, B), np.inf)
    kept = {}

    def candidates(t, logp, tok, par):
        logp = logp.double()
        paths = tok[:t + 1].transpose(1, 2, 0) if own_slot_paths else slot_paths(tok, par, t)
        ban = torch.from_numpy(ban_mask(paths, Vn, cons, rule))
        top_banned[t] = ban.gather(1, torch.topk(logp, k, dim=1).indices).any(1).view(B, W).numpy()
        mass_banned[t] = (logp.exp() * ban).sum(1).view(B, W).numpy()
        if renormalise:
            logp = logp - torch.logsumexp(logp.masked_fill(ban, -np.inf), 1, keepdim=True)
        if after_cut:
            tv, ti = torch.topk(logp, k, dim=1)
            tv = tv.masked_fill(ban.gather(1, ti), -np.inf)
        else:
            tv, ti = torch.topk(logp.masked_fill(ban, -np.inf), k, dim=1)
        kept["tv"] = tv.numpy()
        return tv, ti

    def keep(t, out, cost_t, live):
        live_rec[t] = live
        if W * k > W:                                                         # how far the first candidate left out lies above the last one taken
            flat = np.where(live[:, :, None], cost_t[:, :, None] - kept["tv"].reshape(B, W, k), np.inf).reshape(B, W * k)
            two = np.sort(flat, axis=1)[:, W - 1:W + 1]
            with np.errstate(invalid="ignore"):
                gap[t] = np.where(np.isfinite(two[:, 1]), two[:, 1] - two[:, 0], np.inf)

    rec = orc.free_run(Tn, keep=keep, candidates=candidates)
    return dict(rec, top_banned=top_banned, mass_banned=mass_banned, live=live_rec, gap=gap)


def floor(kind, cell, storage, W, B, vocab, cname, Tn=T):
    """|d nll| of the restatement in fp32 against float64 arithmetic, both teacher-forced on the float64 oracle's own
    constrained free run: what any implementation that accumulates in fp32 is off by"""
    params, feat = decoder_params(kind, cell, vocab, cname), features(kind, B)
    o64 = StepOracle(kind, cell, params, feat, W, storage)
    rec = free_run(o64, CONSTRAINTS[cname], Tn)
    return beam_distance(StepOracle(kind, cell, params, feat, W, storage, torch.float32), o64, rec)["nll"]
