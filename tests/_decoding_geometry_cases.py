"""Cases, inputs, launch arithmetic, oracle, judges, floors and seeded faults for tests/test_gpu_decoding_geometry.py (GPU) and
tests/test_decoding_geometry_inputs.py (CPU): the plain GRU / LSTM decoders' decoding calls -- beam search (device and host
selection, constrained), sample (temperature, top_k, top_p) and scheduled_inputs -- over widths and vocabularies.  Nothing here needs
a GPU.

  CASES         the case table: tests/_decoder_geometry_cases.py's e_wider, h200, h520 and v2049 and two new ones, v_tiny and tall_beam
  problem       (params, feat (B, E)) of one (case, cell, dtype): Y.CASES' scales, <end> boosted by END_BOOST as in
                tests/_decoder_depth_cases.py, bf16-representable for the bf16 kernels
  paths         pure-Python mirror of the launch arithmetic of a decoding call (csrc/decode.hip, csrc/sample.hip, beam.py)
  Walk          one step of the decoder over n rows in float64, rounded to bf16 where the bf16 kernels store (`storage`: R._cells_storage's
                rule), with the seeded faults of the step
  beam_oracle   the walk over (image, slot) rows: the `orc` of tests/_beam_oracle.py's check_records; beam_search its own search
  sample_walk, roll_in    the oracle's own draws (with a fault), or the walk along given tokens
  judge_*       what the GPU test asserts of a call's output, as functions of that output alone: the CPU test hands them the
                output of a faulty oracle and they must raise
  *_floor, FLOORS, bounds   the bf16 bounds: 4 x the distance between the float64 oracle and its bf16-storage replica on these inputs
Every recorded floor is recomputed by tests/test_decoding_geometry_inputs.py, which fails when a recorded figure is stale.
"""
import functools

import numpy as np
import torch

from oracle import restatement as R
from tests import _decoder_geometry_cases as Y
from tests import _nucleus_cases as N
from tests import _scheduled_sampling_cases as K
from tests import test_sample_inputs as I
from tests._beam_oracle import StepOracle, as_recorded, beam_distance, check_records
from tests._decoder_depth_cases import END_BOOST
from tests.test_gpu_decoder_bench_shape import _bf16, _bf16_params

START, END = 1, 2
BEAM_T, SAMPLE_T = 8, 6
FP32_REL = 2e-4             # max |got - ref| / max |ref|, tests/test_gpu_rnn_bptt_fused.py
EXCLUDED = Y.EXCLUDED       # share of steps a comparison may leave out because the oracle's own gap is within rounding
TOP_K, TOP_P = 3, 0.8       # the filtered sample call
SCHED_P = 0.5
CELLS = ("gru", "lstm")

_SCALES = dict(scale=dict(gru=2.0, lstm=3.0), lin=6.0)
# W: the beam widths searched; S: samples per image; sched: caption lengths of the roll-in (None: no roll-in)
CASES = {
    "e_wider": dict(Y.CASES["e_wider"], W=(4, 8), S=2, sched=[8, 7, 5, 3, 1]),
    "h200": dict(Y.CASES["h200"], W=(4, 8), S=2, sched=Y.CASES["h200"]["lens"]),
    "h520": dict(Y.CASES["h520"], W=(4, 8), S=2, sched=None),
    # among 2049 words END_BOOST leaves <end> a probability of a hundredth and no sampled row ends within 6 steps: 5.5 (log 2049 = 7.6)
    "v2049": dict(Y.CASES["v2049"], W=(4, 8), S=2, sched=[8, 8, 7, 6, 5, 4, 3, 2, 1], boost=5.5),
    # V < W at W = 8: k = 5 successors per node, 40 candidates per image, and a first fringe of 5 nodes in 8 slots
    "v_tiny": dict(E=16, H=16, L=1, V=5, lens=[2] * 7, seed=31, W=(4, 8), S=2, sched=None, **_SCALES),
    # B * W = 520 rows per beam step and B * S = 520 rows per sampling step: the two-row-tile cell kernel
    "tall_beam": dict(E=16, H=16, L=1, V=Y.V, lens=[2] * 130, seed=32, W=(4,), S=4, sched=None, **_SCALES),
}
for _c in CASES.values():
    _c["B"] = len(_c["lens"])
SCHED_CASES = tuple(c for c, v in CASES.items() if v["sched"])
CONSTRAINED_CASES = POISON_CASES = ("e_wider", "v2049")
# the constraint set of the constrained search: (min_length, no_repeat_ngram_size, suppress_tokens) -- all three rules
CONSTRAINTS = (3, 2, [0, 1, 5])


@functools.lru_cache(maxsize=None)
def problem(case, cell, bf16):
    """(params, feat (B, E)): read-only"""
    c = CASES[case]
    if case in Y.CASES:
        params, feat = Y.problem(case, cell, False)[:2]
    else:
        params = Y._scaled(R.init_decoder_params(c["E"], c["H"], c["V"], c["L"], cell, seed=c["seed"]), c["scale"][cell], c["lin"])
        feat = torch.randn(c["B"], c["E"], generator=torch.Generator().manual_seed(c["seed"]))
    params = dict(params)
    params["linear.bias"] = params["linear.bias"].clone()
    params["linear.bias"][END] += c.get("boost", END_BOOST)
    if bf16:
        params, feat = _bf16_params(params), _bf16(feat)
    return params, feat


def sample_rows(case, cell, bf16):
    """(feat rows (B * S, E), uniforms (B * S, SAMPLE_T)): row b * S + s is sample s of image b"""
    c = CASES[case]
    return problem(case, cell, bf16)[1].repeat_interleave(c["S"], 0), I.uniforms(c["B"], c["S"], SAMPLE_T).view(-1, SAMPLE_T)


@functools.lru_cache(maxsize=None)
def sched_problem(case):
    """(caption (B, T), lens, uniforms (2, B, T): [0] the coins, [1] the draws)"""
    c = CASES[case]
    cap, lens = Y.captions(c["sched"], c["V"], c["seed"] + 40)
    return cap, lens, torch.rand((2,) + tuple(cap.shape), generator=torch.Generator().manual_seed(c["seed"] + 42))      # (a seed at which about half the valid slots are replaced)


# ====================================================================================================================
# the launch arithmetic
# ====================================================================================================================

SAMPLE_REGS = 256 * 40      # kSampleThreads * kSampleRegs (csrc/sample.hip)


def paths(case, W=None):
    """what a decoding call of the case launches; with W, what a beam search of that width does"""
    c = CASES[case]
    V, H, B = c["V"], c["H"], c["B"]
    pitch = Y.up8(V)
    out = dict(pitch=pitch, train_pitch=Y.vocab_ld(V), pad_columns=pitch - V,
               # st_sample_rows: 16-byte loads need a pitch that is a multiple of 4; the register form a row of at most SAMPLE_REGS
               sample_route="regs" if pitch % 4 == 0 and V <= SAMPLE_REGS else "mem",
               sample_tiles=Y.gemm_launch_tiles(1, B * c["S"]),
               chunks=H // 8,                                   # st_gather_state: 16-byte chunks per gathered bf16 row
               last_unit_tile=H - 16 * ((H - 1) // 16), in0_wider=c["E"] > H)
    if W is not None:
        k = min(W, V)
        out.update(k=k, candidates=W * k, on_device=W * k <= 64,                  # beam.beam_search / st_beam_select
                   topk="threshold" if k <= 8 and k * 256 <= V else "general",     # st_softmax_topk
                   beam_tiles=Y.gemm_launch_tiles(1, B * W))
    return out


def sample_plan(cell, bf16, E, H, L, V, n):
    """make_splan (csrc/sample.hip), the workspace of st_rnn_sample and st_rnn_sched_inputs over n rows: ({region: offset}, bytes).
    Regions h[2], c[2] (LSTM), x, logits, cur, fin in that order, each at a 256-byte boundary: x holds n * E elements beside states of
    L * n * H, the logits n rows at pitch up8(V)"""
    al = lambda v: (v + 255) // 256 * 256
    es = 2 if bf16 else 4
    hb = L * n * H * es
    sizes = [("h0", hb), ("c0", hb if cell != "gru" else 0), ("h1", hb), ("c1", hb if cell != "gru" else 0), ("x", n * E * es),
             ("logits", n * Y.up8(V) * 4), ("cur", n * 8), ("fin", n)]
    off, o = {}, 0
    for k, b in sizes:
        off[k] = o
        o += al(b)
    return off, o


# ====================================================================================================================
# the oracle's step, and what a wrong stride or pitch would make of it
# ====================================================================================================================

# faults of the step (every call runs through them) and of a call's own selection
#   x_pitch_h             the layer-0 input rows (n, E) read at pitch H
#   unit_tail_lost        the units from 64 * floor(H / 64) on stay zero (H no multiple of 64)
#   logits_pitch_train    the logits, written at pitch up8(V), read at pitch st_rnn_vocab_ld(V)
#   child_of_slot0        beam search: a child takes the state of slot 0 of its image, not its parent's
#   last_word_never       the last vocabulary entry is never a candidate / never drawn
#   topk_over_pad         top-k runs over the up8(V) columns of the pitch; the pad columns hold logit 0
FAULTS = ("x_pitch_h", "unit_tail_lost", "logits_pitch_train", "child_of_slot0", "last_word_never", "topk_over_pad")
# (fault) -> the (judge, case) pairs that must reject it in both cells and dtypes
AIMED = {
    "x_pitch_h": (("beam", "e_wider"), ("sample", "e_wider"), ("sched", "e_wider")),
    "unit_tail_lost": (("beam", "h200"), ("beam", "h520"), ("sample", "h200"), ("sample", "h520"), ("sched", "h200")),
    "logits_pitch_train": (("beam", "v2049"), ("sample", "v2049"), ("sched", "v2049")),
    "child_of_slot0": (("beam", "e_wider"), ("beam", "h200"), ("beam", "tall_beam")),
    "last_word_never": (("beam", "v_tiny"), ("sample", "v_tiny")),
    "topk_over_pad": (("beam", "v_tiny"),),
}


class Walk:
    """The decoder of one (case, cell, dtype) stepping n rows in `dt`: R._cells_storage's rounding with `storage` (default: the
    dtype's), and the seeded fault if any.  A state is (h, c), each (L, n, H); c is None for the GRU."""

    def __init__(self, case, cell, bf16, storage=None, fault=None, dt=torch.float64):
        c = CASES[case]
        self.case, self.cell, self.fault = case, cell, fault
        self.st = bool(bf16) if storage is None else storage
        params, self.feat = problem(case, cell, bf16)
        self.p = {k: v.to(dt) for k, v in params.items()}
        self.E, self.H, self.V, self.L = c["E"], c["H"], c["V"], c["L"]

    def _reread(self, rows, width, pitch_w, pitch_r):
        """rows (n, width) laid out at pitch_w (the rest of a row zero), row r read from r * pitch_r"""
        n = rows.shape[0]
        buf = rows.new_zeros(n * max(pitch_w, pitch_r) + width)
        idx = torch.arange(n)[:, None] * pitch_w + torch.arange(width)[None, :]
        buf[idx.reshape(-1)] = rows.reshape(-1)
        return buf[(torch.arange(n)[:, None] * pitch_r + torch.arange(width)[None, :])]

    def _cells(self, x, h, c):
        x = R._store(x, self.st)
        if self.fault == "x_pitch_h":
            x = self._reread(x, self.E, self.E, self.H)
        keep = 64 * (self.H // 64) if self.fault == "unit_tail_lost" else self.H
        hs, cs, inp = [], [], x
        for l in range(self.L):
            w = R._layer_w(self.p, l)
            if self.cell == "gru":
                hl = R._store(R.gru_cell(inp, h[l], *w), self.st)
            else:
                hl, cl = R.lstm_cell(inp, h[l], c[l], *w)
                hl, cl = R._store(hl, self.st), R._store(cl, self.st)
                cl[:, keep:] = 0
                cs.append(cl)
            hl[:, keep:] = 0
            hs.append(hl)
            inp = hl
        logits = inp @ self.p["linear.weight"].t() + self.p["linear.bias"]
        if self.fault == "logits_pitch_train":
            logits = self._reread(logits, self.V, Y.up8(self.V), Y.vocab_ld(self.V))
        return logits, (torch.stack(hs, 0), torch.stack(cs, 0) if cs else None)

    @torch.no_grad()
    def start(self, feat):
        """(logits (n, V), state) of step 0: the image feature from a zero state"""
        feat = feat.to(self.p["linear.bias"].dtype)
        z = feat.new_zeros(self.L, feat.shape[0], self.H)
        return self._cells(feat, z, None if self.cell == "gru" else z)

    @torch.no_grad()
    def step(self, tok, state):
        return self._cells(self.p["embeddings.weight"][torch.as_tensor(tok, dtype=torch.long).reshape(-1)], *state)


def _with_pad(logits, lp):
    """log-probabilities with the pad columns of the pitch appended, holding logit 0"""
    n, V = lp.shape
    pad = (0.0 - torch.logsumexp(logits, 1, keepdim=True)).expand(n, Y.up8(V) - V)
    return torch.cat([lp, pad], 1)


# ====================================================================================================================
# beam search
# ====================================================================================================================

def beam_oracle(walk, feat, W):
    """The walk over fixed (image, slot) rows b * W + w as tests/_beam_oracle.py's StepOracle: every step, the feature step
    included, is the walk's own, with its fault"""
    def step(orc, tok, state):
        orc.logits, new = walk.step(np.asarray(tok).reshape(-1).clip(max=walk.V - 1), state)
        return torch.log_softmax(orc.logits, 1), None, new
    orc = StepOracle("plain", walk.cell, walk.p, feat, W, walk.st, walk.p["linear.bias"].dtype, step)
    orc.state0 = tuple(None if s is None else s.repeat_interleave(W, 1) for s in walk.start(feat)[1])
    return orc


def beam_search(walk, feat, W, T=BEAM_T):
    """the oracle's own search (R.beam_free_run), with the walk's fault of the selection if it has one"""
    orc, fault = beam_oracle(walk, feat, W), walk.fault

    def candidates(t, logp, tok, par):
        k = min(W, logp.shape[1])
        if fault == "last_word_never":
            logp = logp.clone(); logp[:, -1] = -np.inf
        if fault == "topk_over_pad":
            logp = _with_pad(orc.logits, logp)
        return torch.topk(logp, k, dim=1)
    return as_recorded(orc.free_run(T, candidates=candidates,
                                    gather_par=(lambda par: np.where(par >= 0, 0, -1)) if fault == "child_of_slot0" else None))


@functools.lru_cache(maxsize=None)
def oracle_records(case, cell, bf16, W, fault=None):
    return beam_search(Walk(case, cell, bf16, fault=fault), problem(case, cell, bf16)[1], W)


def judge_beam(rec, case, cell, bf16, W, tag="", cons=None):
    """The records of a search walked by the oracle: check_records of tests/_beam_oracle.py (its checks A to C: the number of filled
    slots is counted from the candidates that exist, v_tiny at W = 8 has 5 per node; with `cons`, the ban rule)"""
    V = CASES[case]["V"]
    assert ((rec["tok"] >= 0) & (rec["tok"] < V)).all(), (tag, "a recorded token outside the vocabulary")
    orc = beam_oracle(Walk(case, cell, bf16), problem(case, cell, bf16)[1], W)
    return check_records(rec, orc, beam_bound(case, cell, bf16), tag, cons, hist=rec.get("hist"))


# ====================================================================================================================
# sampling
# ====================================================================================================================

def _draw(lp, u, top_k, top_p):
    """(token, its log-probability under the distribution it was drawn from) by tests/_nucleus_cases.py's rule; without a filter
    the whole vocabulary is kept"""
    if top_k or top_p < 1.0:
        return N.oracle_draw(lp, top_k, top_p, u)
    return N.oracle_draw(lp, 0, 1.0, u, fault="ignored")


def sample_walk(walk, feat, u, ids=None, top_k=0, top_p=1.0):
    """ids None: the oracle draws its own tokens from u (n, T), 0 after <end>; else it walks the given ids (n, T).  Returns (ids,
    logp (n, T) of the draws, lp (n, T, V) full-vocabulary log-probabilities of every step)."""
    n, T, fault = feat.shape[0], u.shape[1], walk.fault
    out, logp, lps = torch.zeros(n, T, dtype=torch.long), torch.zeros(n, T, dtype=torch.float64), []
    fin = torch.zeros(n, dtype=torch.bool)
    logits, state = walk.start(feat)
    for t in range(T):
        lp = torch.log_softmax(logits, 1)
        lps.append(lp)
        if ids is None:
            z = lp
            if fault == "last_word_never":
                z = lp.clone(); z[:, -1] = -float("inf")
            if fault == "topk_over_pad" and top_k:
                z = _with_pad(logits, lp)
            tok, l = _draw(z, u[:, t], top_k, top_p)
            out[:, t] = torch.where(fin, torch.zeros_like(tok), tok)
            logp[:, t] = torch.where(fin, torch.zeros_like(l), l)
        else:
            out[:, t] = ids[:, t]
        fin |= out[:, t] == END
        if t + 1 < T:
            logits, state = walk.step(out[:, t].clamp(max=walk.V - 1), state)
    return out, logp, torch.stack(lps, 1)


@functools.lru_cache(maxsize=None)
def oracle_samples(case, cell, bf16, top_k=0, top_p=1.0, fault=None):
    feat, u = sample_rows(case, cell, bf16)
    return sample_walk(Walk(case, cell, bf16, fault=fault), feat, u, None, top_k, top_p)


def kth_gap(lp, top_k):
    """(n, T) distance between the top_k-th and the next log-probability: a top-k set within rounding of it is undecided"""
    tv = lp.topk(top_k + 1, dim=2).values
    return tv[..., top_k - 1] - tv[..., top_k]


def judge_sample(ids, logp, lengths, case, cell, bf16, top_k=0, top_p=1.0, tag=""):
    """ids, logp (n, T), lengths (n,) of a sample call on sample_rows(case): the oracle walks these tokens.  After <end> come <pad>
    and 0 and `lengths` is the mask's row sum; unfiltered, every draw obeys the interval rule of tests/test_sample_inputs.py and logp
    agrees with the oracle's; filtered, every draw obeys judge_decoder of tests/_nucleus_cases.py.  Where the oracle's top_k-th and
    next entry lie within topk_gap the top-k set is within rounding: fp32 leaves such a step out (at most EXCLUDED of them), bf16
    judges it against either set.  Returns the measured figures."""
    c = CASES[case]
    feat, u = sample_rows(case, cell, bf16)
    n, T = u.shape
    assert ids.shape == logp.shape == (n, T) and lengths.shape == (n,)
    assert ((ids >= 0) & (ids < c["V"])).all(), (tag, "a token outside the vocabulary")
    _, _, lp = sample_walk(Walk(case, cell, bf16), feat, u, ids)
    m = I.checked_mask(ids)
    assert (ids[~m] == 0).all() and (logp[~m] == 0).all() and torch.equal(lengths, m.sum(1)), tag
    d, b = sample_bounds(case, cell, bf16)
    fig = dict(pairs=int(m.sum()), ended=int((lengths < T).sum()), distinct=int(ids[m].unique().numel()), d=d, b=b)
    if not top_k and top_p == 1.0:
        lo, hi = I.interval_excess(lp, ids, u)
        err = (logp.double() - lp.gather(2, ids[..., None]).squeeze(2)).abs()
        fig.update(below=float(lo[m].max()), above=float(hi[m].max()), logp=float(err[m].max()))
        assert (lo[m] <= d).all() and (hi[m] < d).all(), (tag, fig)
        assert (err[m] <= b).all(), (tag, fig)
        return fig
    j = N.judge_decoder(lp, top_k, top_p, ids, logp, u, d, b)
    ok, chk = j["ok"], m.clone()
    if 0 < top_k < c["V"]:
        near = kth_gap(lp, top_k) <= topk_gap(case, cell, bf16)
        if bf16:
            # bf16: entries this close are common (tests/test_decoding_geometry_inputs.py) and nothing is left out: such a draw
            # may obey the judge on either set, the oracle's or the one with the next entry in the top_k-th's place
            tv, ti = lp.topk(top_k + 1, dim=2)
            alt = lp.scatter(2, ti[..., top_k - 1:top_k], tv[..., top_k:] - 1e-9)
            ok = ok | (near & N.judge_decoder(alt, top_k, top_p, ids, logp, u, d, b)["ok"])
            fig["near"] = int((m & near).sum())
        else:
            chk &= ~near
    fig.update(excluded=int((m & ~chk).sum()), u_out=float(torch.maximum(j["below"], j["above"])[chk].max()),
               logp=float(torch.maximum(j["lp_lo"], j["lp_hi"])[chk].max()), failed=int((~ok)[chk].sum()))
    assert fig["excluded"] <= EXCLUDED * fig["pairs"], (tag, fig)
    assert (logp[m] <= N.EPS64).all() and ok[chk].all(), (tag, fig)      # (EPS64: the float64 oracle judged by itself)
    return fig


# ====================================================================================================================
# scheduled sampling's roll-in
# ====================================================================================================================

def roll_in(walk, case, ids=None):
    """tests/_scheduled_sampling_cases.py's roll_in for the plain decoders on sched_problem(case): ids None: the oracle mixes its own
    tokens, else it walks the given input ids.  Returns (input_ids (B, T), replaced (B, T), lp (B, T, V): lp[:, j] decides slot j)."""
    cap, lens, u = sched_problem(case)
    B, T = cap.shape
    rep = torch.from_numpy(K.mix_rule("rnn", lens, u[0].numpy(), SCHED_P))
    out = cap.clone() if ids is None else ids.clone()
    lps = torch.zeros(B, T, walk.V, dtype=torch.float64)
    logits, state = walk.start(walk.feat)
    for j in range(max(lens) - 1):
        lp = torch.log_softmax(logits, 1)
        lps[:, j] = lp
        if ids is None:
            z = lp
            if walk.fault == "last_word_never":
                z = lp.clone(); z[:, -1] = -float("inf")
            out[:, j] = torch.where(rep[:, j], _draw(z, u[1][:, j], 0, 1.0)[0], out[:, j])
        if j + 1 < max(lens) - 1:
            logits, state = walk.step(out[:, j], state)
    return out, rep, lps


@functools.lru_cache(maxsize=None)
def oracle_roll_in(case, cell, bf16, fault=None):
    return roll_in(Walk(case, cell, bf16, fault=fault), case)


def judge_sched(ids, rep, case, cell, bf16, tag=""):
    """`replaced` is the mix rule exactly, the ids are the caption's wherever nothing was replaced, and every replaced slot obeys the
    interval rule against the oracle's walk of these same ids"""
    cap, lens, u = sched_problem(case)
    assert ids.shape == rep.shape == cap.shape and ((ids >= 0) & (ids < CASES[case]["V"])).all(), tag
    want = torch.from_numpy(K.mix_rule("rnn", lens, u[0].numpy(), SCHED_P))
    assert torch.equal(rep, want), (tag, "replaced is not (coin < p) & valid")
    assert torch.equal(ids[~rep], cap[~rep]), (tag, "an unreplaced slot differs from the caption")
    _, _, lp = roll_in(Walk(case, cell, bf16), case, ids)
    lo, hi = K.interval_excess(lp, ids, u[1])
    d = sched_bound(case, cell, bf16)
    fig = dict(replaced=int(rep.sum()), valid=int(K.valid_slots("rnn", lens, cap.shape[1]).sum()), differ=int((ids != cap).sum()),
               below=float(lo[want].max()), above=float(hi[want].max()), d=d)
    assert (lo[want] <= d).all() and (hi[want] < d).all(), (tag, fig)
    return fig


# ====================================================================================================================
# bounds
# ====================================================================================================================

@functools.lru_cache(maxsize=None)
def logit_scale(case, cell):
    """max |logit| along the float64 oracle's own samples on the fp32 inputs: the scale FP32_REL refers to"""
    feat, u = sample_rows(case, cell, False)
    w = Walk(case, cell, False)
    ids = oracle_samples(case, cell, False)[0]
    worst, (logits, state) = 0.0, w.start(feat)
    for t in range(SAMPLE_T):
        worst = max(worst, logits.abs().max().item())
        if t + 1 < SAMPLE_T:
            logits, state = w.step(ids[:, t], state)
    return worst


@functools.lru_cache(maxsize=None)
def beam_floor(case, cell):
    """largest |d log p| of a recorded (parent, token) between the float64 oracle and its bf16-storage replica, both on the
    bf16-representable inputs and both following the replica's own search, over the case's beam widths"""
    feat = problem(case, cell, True)[1]
    return max(beam_distance(beam_oracle(Walk(case, cell, True), feat, W), beam_oracle(Walk(case, cell, True, storage=False), feat, W),
                             oracle_records(case, cell, True, W))["nll"] for W in CASES[case]["W"])


@functools.lru_cache(maxsize=None)
def sample_floor(case, cell):
    """(CDF, log-probability of the token) between the float64 oracle and its bf16-storage replica along the replica's own draws"""
    feat, u = sample_rows(case, cell, True)
    ids, _, lp_st = oracle_samples(case, cell, True)
    _, _, lp_pl = sample_walk(Walk(case, cell, True, storage=False), feat, u, ids)
    m = I.checked_mask(ids)
    tok = ids[..., None]
    return (float((lp_st.exp().cumsum(2) - lp_pl.exp().cumsum(2)).abs()[m].max()),
            float((lp_st.gather(2, tok) - lp_pl.gather(2, tok)).abs().squeeze(2)[m].max()))


@functools.lru_cache(maxsize=None)
def sched_floor(case, cell):
    """CDF distance between the float64 oracle and its bf16-storage replica along the replica's own mixed ids, over the valid slots"""
    cap, lens, _ = sched_problem(case)
    ids, _, lp_st = oracle_roll_in(case, cell, True)
    _, _, lp_pl = roll_in(Walk(case, cell, True, storage=False), case, ids)
    m = torch.from_numpy(K.valid_slots("rnn", lens, cap.shape[1]))
    return float((lp_st.exp().cumsum(2) - lp_pl.exp().cumsum(2)).abs()[m].max())


# (case, cell) -> beam_floor; the beam NLL_ABS of the bf16 kernels is 4 x it
BEAM_FLOORS = {
    ('e_wider', 'gru'): 1.14e-02,
    ('e_wider', 'lstm'): 6.11e-03,
    ('h200', 'gru'): 1.20e-02,
    ('h200', 'lstm'): 6.32e-03,
    ('h520', 'gru'): 1.36e-02,
    ('h520', 'lstm'): 5.40e-03,
    ('v2049', 'gru'): 5.09e-03,
    ('v2049', 'lstm'): 3.04e-03,
    ('v_tiny', 'gru'): 1.37e-02,
    ('v_tiny', 'lstm'): 8.08e-03,
    ('tall_beam', 'gru'): 1.04e-02,
    ('tall_beam', 'lstm'): 7.51e-03,
}
# (case, cell) -> sample_floor; the bf16 sampling d and logp bounds are 4 x these
SAMPLE_FLOORS = {
    ('e_wider', 'gru'): (1.73e-03, 5.52e-03),
    ('e_wider', 'lstm'): (4.78e-04, 2.09e-03),
    ('h200', 'gru'): (1.98e-03, 8.14e-03),
    ('h200', 'lstm'): (7.10e-04, 4.45e-03),
    ('h520', 'gru'): (1.11e-03, 7.92e-03),
    ('h520', 'lstm'): (7.50e-04, 2.30e-03),
    ('v2049', 'gru'): (6.51e-04, 4.22e-03),
    ('v2049', 'lstm'): (4.11e-04, 2.18e-03),
    ('v_tiny', 'gru'): (8.34e-04, 4.52e-03),
    ('v_tiny', 'lstm'): (5.81e-04, 2.31e-03),
    ('tall_beam', 'gru'): (1.86e-03, 1.19e-02),
    ('tall_beam', 'lstm'): (1.00e-03, 5.85e-03),
}
# (case, cell) -> sched_floor; the bf16 roll-in d is 4 x it
SCHED_FLOORS = {
    ('e_wider', 'gru'): 1.44e-03,
    ('e_wider', 'lstm'): 5.26e-04,
    ('h200', 'gru'): 1.33e-03,
    ('h200', 'lstm'): 8.85e-04,
    ('v2049', 'gru'): 3.74e-04,
    ('v2049', 'lstm'): 2.91e-04,
}


def beam_bound(case, cell, bf16):
    """NLL_ABS of check_records, for words and <end> alike"""
    return 4 * BEAM_FLOORS[(case, cell)] if bf16 else FP32_REL * logit_scale(case, cell)


def sample_bounds(case, cell, bf16):
    """(d of the interval rule: a probability, of scale 1; the logp bound)"""
    if not bf16:
        return FP32_REL, FP32_REL * logit_scale(case, cell)
    return tuple(4 * f for f in SAMPLE_FLOORS[(case, cell)])


def sched_bound(case, cell, bf16):
    return 4 * SCHED_FLOORS[(case, cell)] if bf16 else FP32_REL


def topk_gap(case, cell, bf16):
    """the top_k-th and the next entry are told apart beyond this: fp32 Y.FP32_GAP, bf16 the logp bound (what a log-probability
    may be off by)"""
    return sample_bounds(case, cell, True)[1] if bf16 else Y.FP32_GAP[cell]
