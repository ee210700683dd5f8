"""Nucleus (top-p) sampling: the float64 oracle, the judge and the inputs that tests/test_gpu_nucleus.py (GPU) and
tests/test_nucleus_inputs.py (CPU) share.  Nothing here needs a GPU.

The rule (include/showtell_hip.h, st_sample_rows_topp).  z = logits * inv_temperature; with top_k > 0 only the top-k set is
eligible and probabilities are renormalised over it; the eligible entries are ordered by value descending, the lowest index
first among equal values; c_excl(j) is the mass strictly before entry j in that order and j is kept iff c_excl(j) < top_p.
The token is drawn among the kept entries in index order, logp is its log-probability under the kept distribution.

The judge.  fp32 sums cannot decide an entry whose c_excl lies within rounding of top_p, so a draw is judged against a RANGE
of prefixes: m_lo and m_hi are the prefix sizes of the rule at top_p - d and top_p + d, C[m] the mass of the first m entries,
A(m) the mass of the entries of prefix m with an index below the token, p the token's probability.  A draw passes iff
  (i)   the token is inside prefix m_hi,
  (ii)  lp(tok) - log C[m_hi] - b <= logp <= lp(tok) - log C[m_lo] + b,
  (iii) A(m_lo) / C[m_hi] - d <= u < (A(m_hi) + p) / C[m_lo] + d.
With m_lo == m_hi this is the interval rule of tests/test_gpu_sample.py over the oracle's nucleus."""
import numpy as np
import torch

from tests import test_gpu_sample as GS
from tests import test_sample_inputs as I

EPS64 = 1e-12     # the float64 oracle's own rounding (log C[m] of a one-word nucleus is log(exp(lp)), not lp): where b is 0
NEAR_ONE = float(np.nextafter(np.float32(1), np.float32(0)))

# (temperature, top_k, top_p) of part A
A_CASES = [(1.0, 0, 0.9), (0.7, 0, 0.5), (1.3, 0, 0.95), (3.0, 0, 0.9), (1.0, 32, 0.8), (1.0, 5, 0.5), (1.0, 0, 1e-6)]
# (V, ld) of part B: scalar loads, 16-byte loads beyond the register form
ROUTES = [(5003, 5003), (10243, 10244)]
# (kind, cell, storage, shape, top_k, top_p) of parts D and E; temperature 1.0, boost False
DECODER_CASES = ([("plain", cell, storage, (23, 11), 0, p) for cell in ("gru", "lstm") for storage in (True, False) for p in (0.9, 0.5)]
                 + [("plain", "gru", True, (23, 11), 20, 0.9)]
                 + [("attn", cell, True, (24, 3), 0, 0.9) for cell in ("gru", "lstm")])

TIE_AT = (4000, 100, 2000, 3000)       # the boundary-tie row: log 0.4 at 4000, log 0.2 at 100, 2000, 3000; top_p = 0.7
TIE_P = 0.7


class Ordered:
    """The eligible distribution of every row of z (N, V) float64 in the rule's order."""

    def __init__(self, z, top_k, higher_index_first=False):
        z = z.double()
        N, V = z.shape
        if higher_index_first:             # (a seeded fault) among equal values the HIGHEST index first
            order = (V - 1) - torch.sort(z.flip(1), dim=1, descending=True, stable=True).indices
        else:
            order = torch.sort(z, dim=1, descending=True, stable=True).indices
        self.elig = torch.ones(N, V, dtype=torch.bool)
        if top_k:
            self.elig = torch.zeros(N, V, dtype=torch.bool).scatter_(1, order[:, :top_k], True)
            z = torch.where(self.elig, z, torch.full_like(z, -float("inf")))
        self.order = order
        self.rank = torch.empty_like(order).scatter_(1, order, torch.arange(V).expand(N, V).contiguous())
        self.lp = torch.log_softmax(z, 1)                      # over the eligible set, -inf outside
        self.p = self.lp.exp()
        ps = self.p.gather(1, order)
        self.c_incl = ps.cumsum(1)                             # sorted order
        self.c_excl = torch.cat([torch.zeros(N, 1, dtype=torch.float64), self.c_incl[:, :-1]], 1)

    def prefix(self, top_p, inclusive=False):
        """size of the kept prefix per row: entries with c_excl < top_p (top_p scalar or (N,)); never below 1"""
        tp = torch.as_tensor(top_p, dtype=torch.float64).reshape(-1, 1)
        kept = (self.c_incl <= tp) if inclusive else (self.c_excl < tp)
        return kept.sum(1).clamp(min=1)

    def mass(self, m):
        return self.c_incl.gather(1, (m - 1)[:, None])[:, 0]

    def kept(self, m):
        return self.rank < m[:, None]


def scaled(rows, inv_t):
    """fp32 logits times the fp32 inverse temperature, exactly, in float64 (24 x 24 bits: the order of the rows survives)"""
    return rows.double() * float(inv_t)


def nucleus(rows, inv_t, top_k, top_p):
    """(lp (N, V) float64 over the full or top-k set, order (N, V), c_excl (N, V) in the rule's order, kept mask (N, V))"""
    o = Ordered(scaled(rows, inv_t), top_k)
    return o.lp, o.order, o.c_excl, o.kept(o.prefix(top_p))


def draw_from(p_kept, u):
    """the smallest index whose inclusive cumulative probability over the (unnormalised) kept masses exceeds u * total"""
    c = p_kept.cumsum(1)
    tok = (c <= u.double()[:, None] * c[:, -1:]).sum(1)
    last = (p_kept > 0).long().mul(torch.arange(1, p_kept.shape[1] + 1)).max(1).values - 1
    return torch.minimum(tok, last)


def oracle_draw(z, top_k, top_p, u, fault=None):
    """(tok (N,), logp (N,)) of the rule in float64, or of a seeded fault:
    'inclusive' keep iff c_incl <= top_p; 'high_tie' ties by the higher index; 'p_before_k' top-p on the full distribution,
    then top-k; 'raw_logp' logp of the full vocabulary; 'next_u' the next row's u; 'ignored' top_p ignored"""
    z = z.double()
    if fault == "next_u":
        u = u.roll(-1, 0)
    if fault == "p_before_k" and top_k:
        full, cut = Ordered(z, 0), Ordered(z, top_k)
        keep = full.kept(full.prefix(top_p)) & cut.elig
        o = full
    else:
        o = Ordered(z, top_k, higher_index_first=fault == "high_tie")
        keep = o.kept(o.prefix(1.0 if fault == "ignored" else top_p, inclusive=fault == "inclusive"))
        if fault == "ignored":
            keep = o.elig
    pk = torch.where(keep, o.p, torch.zeros_like(o.p))
    tok = draw_from(pk, u)
    lp_tok = o.lp.gather(1, tok[:, None])[:, 0]
    logp = lp_tok - pk.sum(1).log()
    if fault == "raw_logp":
        logp = torch.log_softmax(z, 1).gather(1, tok[:, None])[:, 0]
    return tok, logp


def judge(z, top_k, top_p, tok, logp, u, d, b):
    """Every row of z (N, V) judged; returns a dict: ok (N,) bool and, for the MEASURE lines, how far each condition is from
    its limit WITHOUT the tolerance (<= 0: inside the oracle's own range): below = A(m_lo) / C[m_hi] - u,
    above = u - (A(m_hi) + p) / C[m_lo], lp_lo = (lp - log C[m_hi]) - logp, lp_hi = logp - (lp - log C[m_lo])."""
    o = Ordered(z, top_k)
    N, V = o.p.shape
    tok, u, logp = tok.long().reshape(N), u.double().reshape(N), logp.double().reshape(N)
    m_lo, m_hi = o.prefix(top_p - d), o.prefix(top_p + d)
    C_lo, C_hi = o.mass(m_lo), o.mass(m_hi)
    inside = o.rank.gather(1, tok[:, None])[:, 0] < m_hi
    lp_tok = o.lp.gather(1, tok[:, None])[:, 0]
    p_tok = lp_tok.exp()
    before = torch.arange(V)[None, :] < tok[:, None]
    A_lo = torch.where(o.kept(m_lo) & before, o.p, torch.zeros_like(o.p)).sum(1)
    A_hi = torch.where(o.kept(m_hi) & before, o.p, torch.zeros_like(o.p)).sum(1)
    below, above = A_lo / C_hi - u, u - (A_hi + p_tok) / C_lo
    lp_lo, lp_hi = (lp_tok - C_hi.log()) - logp, logp - (lp_tok - C_lo.log())
    ok = inside & (below <= d) & (above < d) & (lp_lo <= b + EPS64) & (lp_hi <= b + EPS64)
    return dict(ok=ok, inside=inside, below=below, above=above, lp_lo=lp_lo, lp_hi=lp_hi, m_lo=m_lo, m_hi=m_hi, C_lo=C_lo, C_hi=C_hi)


def measure_line(tag, j, live, d, b):
    f = lambda x: float(x[live].max())
    return (f"MEASURE {tag}: u outside the oracle's range by {max(f(j['below']), f(j['above'])):.2e} (d {d:.2e}); logp outside by "
            f"{max(f(j['lp_lo']), f(j['lp_hi'])):.2e} (b {b:.2e}); rows with m_lo < m_hi: {int((j['m_lo'] < j['m_hi'])[live].sum())} "
            f"of {int(live.sum())}")


# ---- the fp32 floors the bounds come from -----------------------------------------------------------------------------------

def floors(rows, inv_t, top_k, top_p):
    """(cdf, logp): the largest distance between a sequential float32 evaluation and the float64 one on these rows -- the
    cumulative sum in the rule's descending order, the CDF in index order over the kept set, the kept set's log-probabilities"""
    o = Ordered(scaled(rows, inv_t), top_k)
    keep = o.kept(o.prefix(top_p))
    z32 = rows.float() * torch.tensor(inv_t, dtype=torch.float32)
    ninf = torch.full_like(z32, -float("inf"))
    p32 = torch.softmax(torch.where(o.elig, z32, ninf), 1)
    desc = np.cumsum(p32.gather(1, o.order).numpy(), axis=1, dtype=np.float32).astype(np.float64)
    d1 = np.abs(desc - o.c_incl.numpy()).max()
    zk32 = torch.where(keep, z32, ninf)
    zk64 = torch.where(keep, scaled(rows, inv_t), ninf.double())
    cdf32 = np.cumsum(torch.softmax(zk32, 1).numpy(), axis=1, dtype=np.float32).astype(np.float64)
    d2 = np.abs(cdf32 - torch.softmax(zk64, 1).cumsum(1).numpy()).max()
    ok = keep & torch.isfinite(zk64)
    lpd = (torch.log_softmax(zk32, 1).double() - torch.log_softmax(zk64, 1))[ok].abs().max()
    return float(max(d1, d2)), float(lpd)


# ---- inputs -----------------------------------------------------------------------------------------------------------------

def a_inputs():
    """The 44 rows of tests/test_gpu_sample.py::rows_inputs three times: with their own u, with u = 0 and with
    u = nextafter(1, 0) -- the two added copies draw the first and the last kept index.  (logits (132, ld), u, finished, names:
    row r of the original is rows r, r + 44, r + 88)"""
    logits, u, fin, names = GS.rows_inputs()
    n = logits.shape[0]
    uu = torch.cat([u, torch.zeros(n), torch.full((n,), NEAR_ONE)]).float()
    return logits.repeat(3, 1), uu, fin.repeat(3), names, n


def tie_inputs():
    """One row three times (u = 0.5, 0, -> 1): -inf everywhere but log 0.4 at 4000 and log 0.2 at 100, 2000, 3000"""
    row = torch.full((1, GS.ROWS_LD), 1e4)
    row[0, :GS.ROWS_V] = -float("inf")
    row[0, TIE_AT[0]] = float(np.log(0.4))
    row[0, list(TIE_AT[1:])] = float(np.log(0.2))
    return row.repeat(3, 1), torch.tensor([0.5, 0.0, NEAR_ONE]), torch.zeros(3, dtype=torch.uint8)


def route_rows(V, ld):
    """route_inputs of tests/test_gpu_sample.py with the constant last row a second time at u -> 1 (13 rows)"""
    logits, u, fin = GS.route_inputs(V, ld)
    return torch.cat([logits, logits[11:]], 0), torch.cat([u, torch.tensor([NEAR_ONE])]).float(), torch.zeros(13, dtype=torch.uint8)


def small_rows(V):
    g = torch.Generator().manual_seed(100 + V)
    ld = (V + 7) // 8 * 8
    logits = torch.full((5, ld), 1e4)
    logits[:, :V] = torch.randn(5, V, generator=g) * 3
    return logits, torch.rand(5, generator=g), torch.zeros(5, dtype=torch.uint8)


# ---- the decoders' oracle, free running under the rule (or a fault) -----------------------------------------------------------

_CACHE = {}


def decoder_walk(kind, cell, storage, shape, top_k, top_p, fault=None):
    """The storage oracle of tests/test_sample_inputs.py drawing its OWN tokens by `oracle_draw`: (ids (n, T), logp (n, T) of the
    draws, lp (n, T, V) full-vocabulary log-probabilities, u (n, T))"""
    key = (kind, cell, storage, shape, top_k, top_p, fault)
    if key in _CACHE:
        return _CACHE[key]
    from oracle import restatement as R
    Bn, S = shape
    T, END, START = I.T, I.END, I.START
    orc = I.Oracle(kind, cell, I.decoder_params(kind, cell, False, 1.0), I.features(kind, Bn), S, storage)
    u = I.uniforms(Bn, S).view(Bn * S, T)
    p, n, st = orc.p, orc.n, storage
    ids, logp, lps = torch.zeros(n, T, dtype=torch.long), torch.zeros(n, T, dtype=torch.float64), []
    fin = torch.zeros(n, dtype=torch.bool)
    with torch.no_grad():
        if kind == "plain":
            Ln, Hd = R.num_layers_of(p), p["unit.weight_hh_l0"].shape[1]
            h = orc.feat.new_zeros(Ln, n, Hd)
            c = orc.feat.new_zeros(Ln, n, Hd) if cell != "gru" else None
            top, h, c = R._cells_storage(p, R._store(orc.feat, st), h, c, cell, st)
            raw, state = top @ p["linear.weight"].t() + p["linear.bias"], (h, c)
        else:
            ctx, state = R.attn_beam_init_bf16_storage(p, orc.feat, 1, cell, st)
            raw, _, state = R.attn_beam_step_bf16_storage(p, ctx, torch.full((n, 1), START), state, None, cell, st)
        for t in range(T):
            lp = torch.log_softmax(raw, 1)
            lps.append(lp)
            tok, l = oracle_draw(lp, top_k, top_p, u[:, t], fault)
            ids[:, t] = torch.where(fin, torch.zeros_like(tok), tok)
            logp[:, t] = torch.where(fin, torch.zeros_like(l), l)
            fin |= ids[:, t] == END
            if t + 1 == T:
                break
            if kind == "plain":
                raw, state = R.rnn_beam_step_bf16_storage(p, ids[:, t].view(n, 1), state, None, cell, st)
            else:
                raw, _, state = R.attn_beam_step_bf16_storage(p, ctx, ids[:, t].view(n, 1), state, None, cell, st)
    _CACHE[key] = (ids, logp, torch.stack(lps, 1), u)
    return _CACHE[key]


def judge_decoder(lp, top_k, top_p, ids, logp, u, d, b):
    """`judge` on every (row, step) of lp (n, T, V); the dict's entries come back as (n, T)"""
    n, T, V = lp.shape
    j = judge(lp.reshape(n * T, V), top_k, top_p, ids.reshape(-1), logp.reshape(-1), u.reshape(-1), d, b)
    return {k: v.view(n, T) for k, v in j.items()}
