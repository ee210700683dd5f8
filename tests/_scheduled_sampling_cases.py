"""The cases, the numpy replica of the mix rule, the float64 oracles, the bounds and the seeded faults that
tests/test_gpu_scheduled_sampling.py and tests/test_scheduled_sampling_inputs.py share.

Semantics (include/showtell_hip.h, st_rnn_sched_inputs / st_attn_sched_inputs).  input_ids is a copy of the caption in which slot
(b, j) holds the model's own draw iff the packed forward reads the slot and coin[b, j] < p (strict):
  plain decoders      slot j feeds step j + 1: read iff j + 1 < lens[b]; drawn from step j's logits
  attention decoders  slot j feeds step j:     read iff 1 <= j < lens[b] (slot 0 is <start>); drawn from step j - 1's logits
The draw is st_sample_rows' rule on draw_u[b, j]: the smallest v whose inclusive cumulative probability exceeds u.

Cases: the shapes of tests/_label_smoothing_cases.py (gru777, lstm1500, gru130 in bf16 with E = H = 512; gru_fp32; the fp32
attention fixture) with the captions' last two rows cut to lengths 2 and 1 (the padding zeroed), so that a row has no slot to
replace (plain, length 1; attention, length 1) or exactly one (plain, length 2).
  roll-in   the case's parameters with `linear.weight` scaled (SHARPEN): at the seeded initial weights every step's distribution is
            nearly uniform and nearly the same, so a draw taken from the wrong step's logits would pass the interval rule.
  loss      the parameters of tests/_label_smoothing_cases.py as they are (its gradient bounds were made for them).

Oracles.  Roll-in: oracle/restatement.py's storage restatement at W = 1 (the one tests/test_sample_inputs.py uses), float64,
bf16 storage for the bf16 cases.  `roll_in` draws its own tokens (and takes a seeded fault) or, given input ids, walks them
teacher-forced.  Loss: a double nn.GRU / nn.LSTM on embeddings(X) (R.attn_forward with inputs X for the attention case), cross entropy
against the packed caption; with dropout, the layer walk of tests/_dropout_cases.py with that file's replica of the masks.
Every reference is computed once per process (lru_cache) and handed out as is: callers do not modify it.

Bounds (none comes from the code under test).
  interval rule   c_lo - d <= u < c_hi + d, d = 4 x FLOORS[case]: the distance between the SAME storage restatement in fp32 and in
                  float64 arithmetic (sequential float32 cumulative sum against the float64 one), teacher-forced on the float64
                  oracle's own mixed ids: the rule of tests/test_gpu_sample.py.  `python -m tests._scheduled_sampling_cases`
                  prints the floors (CPU only).
  gradients       the linear form of tests/_weighted_loss_cases.py, tol * (max|g_ref(w+)| + max|g_ref(w-)|), GRAD_TOL.
  loss            2e-2 * max(mean|w|, ..) for bf16, 1e-4 (+ 3e-5 for the attention decoder's unweighted term) for fp32: the bounds
                  of tests/test_gpu_weighted_loss.py / tests/test_gpu_label_smoothing.py."""
import functools

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import restatement as R
from tests import _dropout_cases as D
from tests import _label_smoothing_cases as S
from tests import _weighted_loss_cases as W
from tests._beam_oracle import StepOracle

CASES = {k: S.CASES[k] for k in ("gru777", "lstm1500", "gru130", "gru_fp32", "attn_fp32")}
ROUTES = S.ROUTES                           # (case, ST_FUSED_CE): gru777 also on the launch chain
GRAD_TOL = W.GRAD_TOL
ZERO_GRADS = W.ZERO_GRADS
P = 0.5                                     # the rate of every roll-in case
# scale of linear.weight for the roll-in (chosen on the CPU so that the 'wrong step' fault fails the interval rule)
SHARPEN = {"gru777": 60.0, "lstm1500": 200.0, "gru130": 30.0, "gru_fp32": 40.0, "attn_fp32": 40.0}
# FLOORS[case] = CDF distance between fp32 and float64 arithmetic of the storage restatement (`python -m tests._scheduled_sampling_cases`)
FLOORS = {
    "gru777": 3.65e-03,
    "lstm1500": 1.88e-03,
    "gru130": 2.06e-04,
    "gru_fp32": 1.21e-06,
    "attn_fp32": 3.87e-07,
}
DROPOUT = dict(p=(0.5, 0.4, 0.6), seed=(0xFEDCBA98 << 32) | 0x76543210)      # the dropout run of the loss test (gru777)
LABEL_SMOOTHING = S.EPS


def family(case):
    return CASES[case][0]


def cell_of(case):
    return CASES[case][1]


def dtype_name(case):
    return CASES[case][2]


def torch_dtype(case):
    return torch.bfloat16 if dtype_name(case) == "bf16" else torch.float32


def storage(case):
    return dtype_name(case) == "bf16"


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(params, feat, caption, lens, alpha_c): tests/_label_smoothing_cases.py's with the last two rows cut to lengths 2 and 1."""
    params, feat, cap, lens, alpha_c = S.inputs(case)
    lens = list(lens)
    lens[-2], lens[-1] = 2, 1
    cap = cap.clone()
    for b in (-2, -1):
        cap[b, lens[b]:] = 0
    assert all(lens[i] >= lens[i + 1] for i in range(len(lens) - 1))
    return params, feat, cap, lens, alpha_c


@functools.lru_cache(maxsize=None)
def rollin_params(case):
    params = {k: v.clone() for k, v in inputs(case)[0].items()}
    params["linear.weight"] = params["linear.weight"] * SHARPEN[case]
    if storage(case):
        params = {k: v.bfloat16().float() for k, v in params.items()}
    return params


@functools.lru_cache(maxsize=None)
def uniforms(case, seed=23):
    """(2, B, T) fp32 in [0, 1): [0] the coins, [1] the draws."""
    cap = inputs(case)[2]
    return torch.rand((2,) + tuple(cap.shape), generator=torch.Generator().manual_seed(seed + len(case)))


@functools.lru_cache(maxsize=None)
def attn_lstm_inputs():
    """The LSTM attention fixture with the captions cut as in `inputs` and the projection sharpened as for the roll-in: the fourth
    cell of the p = 1 comparison with ``sample`` (test 2), which needs no oracle."""
    from tests._util import load_fixture
    params, _, d = load_fixture("attn_lstm_small.npz")
    lens = d["lens"].tolist()
    lens[-2], lens[-1] = 2, 1
    cap = torch.from_numpy(d["caption"]).clone()
    for b in (-2, -1):
        cap[b, lens[b]:] = 0
    params = {k: v.clone() for k, v in params.items()}
    params["linear.weight"] = params["linear.weight"] * SHARPEN["attn_fp32"]
    return params, torch.from_numpy(d["feat"]), cap, lens


# ---- the mix rule, numpy ---------------------------------------------------------------------------------------------------

def valid_slots(kind, lens, T):
    """(B, T) bool: the slots the packed forward reads and the roll-in may replace."""
    j = np.arange(T)[None, :]
    ln = np.asarray(lens)[:, None]
    return (j + 1 < ln) if kind == "rnn" else ((j >= 1) & (j < ln))


def mix_rule(kind, lens, coin, p):
    """replaced (B, T) bool = valid & (coin < p), the comparison in float32 as the kernel makes it."""
    coin = np.asarray(coin, dtype=np.float32)
    return valid_slots(kind, lens, coin.shape[1]) & (coin < np.float32(p))


def mix_tokens(caption, drawn, replaced):
    """input_ids: the drawn token where replaced, the caption's everywhere else."""
    return np.where(replaced, drawn, caption)


# ---- the roll-in oracle ----------------------------------------------------------------------------------------------------

FAULTS = ("flipped", "shifted", "past_length", "wrong_step")


def walker(kind, cell, params, feat, st, dt=torch.float64):
    """The storage restatement stepping all B rows (W = 1) in `dt`: (start, step).  start() -> (plain: the log-probabilities of the
    feature step, attention: None; the state after it / the root state); step(tok (B,), state) -> (log-probabilities, new state)."""
    orc = StepOracle("plain" if kind == "rnn" else "attn", cell, params, feat, 1, st, dt)

    def start():
        logits, state = orc.start()
        return (None if logits is None else torch.log_softmax(logits, 1)), state

    def step(tok, state):
        lp, _, state = orc.step(tok.view(orc.B, 1), state)
        return lp, state
    return start, step


def _draw(lp, u):
    cdf = lp.exp().cumsum(1)
    return (cdf <= u.to(cdf.dtype)[:, None]).sum(1).clamp(max=lp.shape[1] - 1)


def roll_in(case, p=P, u=None, fault=None, ids=None, dt=torch.float64):
    """The sequential roll-in in `dt`.  ids None: the oracle mixes its own tokens (free running, with the seeded `fault` if any);
    else it walks the given input ids.  Returns (input_ids (B, T), replaced (B, T) bool, lp (B, T, V)): lp[b, j] is the
    log-probability row slot j is drawn from (zeros where no step produces one).
    Faults: 'flipped' replaces iff coin >= p; 'shifted' writes the draw of slot j to slot j + 1; 'past_length' ignores the lengths;
    'wrong_step' draws from the logits one step off (the stale buffer of the launch before: a sequential roll-in has no later
    logits to read), uniform where there is none."""
    _, _, cap, lens, _ = inputs(case)
    kind = family(case)
    u = uniforms(case) if u is None else u
    coin, du = u[0], u[1]
    B, T = cap.shape
    start, step = walker(kind, cell_of(case), rollin_params(case), inputs(case)[1], storage(case), dt)
    Vn = rollin_params(case)["linear.weight"].shape[0]
    valid = torch.from_numpy(valid_slots(kind, lens if fault != "past_length" else [T + 1] * B, T))
    fire = (coin < np.float32(p)) if fault != "flipped" else ~(coin < np.float32(p))
    rep = valid & fire
    out = cap.clone() if ids is None else ids.clone()
    replaced = torch.zeros(B, T, dtype=torch.bool)
    lps = torch.zeros(B, T, Vn, dtype=dt)
    with torch.no_grad():
        lp, state = start()
        prev = torch.full((B, Vn), -float(np.log(Vn)), dtype=dt)
        first = 0 if kind == "rnn" else 1                  # the first slot a step's logits decide
        if kind != "rnn":
            lp, state = step(out[:, 0], state)
        for j in range(first, max(lens) - 1 + first):
            lps[:, j] = lp
            if ids is None:
                tok = _draw(prev if fault == "wrong_step" else lp, du[:, j])
                dst = j + 1 if fault == "shifted" else j
                if dst < T:
                    out[:, dst] = torch.where(rep[:, j], tok, out[:, dst])
                    replaced[:, dst] |= rep[:, j]
            prev = lp
            if j + 1 < max(lens) - 1 + first:
                lp, state = step(out[:, j], state)
    if ids is not None:
        replaced = rep
    return out, replaced, lps


@functools.lru_cache(maxsize=None)
def oracle_roll_in(case, fault=None):
    return roll_in(case, fault=fault)


def interval_excess(lp, ids, u):
    """tests/test_sample_inputs.py's rule per slot: (c_lo - u, u - c_hi), both <= 0 inside the oracle's own interval."""
    p = lp.double().exp()
    c_hi = p.cumsum(2).gather(2, ids[..., None]).squeeze(2)
    c_lo = c_hi - p.gather(2, ids[..., None]).squeeze(2)
    u = u.double()
    return c_lo - u, u - c_hi


def d_bound(case):
    return 4.0 * FLOORS[case]


def rollin_violations(case, input_ids, replaced, p=P, u=None):
    """What test 3 asserts, as a list of findings (empty: passes): `replaced` is the rule exactly, input_ids is the caption wherever
    it is not replaced, and every replaced slot obeys the interval rule against the oracle's walk of these same input ids."""
    _, _, cap, lens, _ = inputs(case)
    u = uniforms(case) if u is None else u
    want = torch.from_numpy(mix_rule(family(case), lens, u[0].numpy(), p))
    out = []
    if not torch.equal(replaced, want):
        out.append(f"replaced differs from (coin < p) & valid in {int((replaced != want).sum())} slots")
    if not torch.equal(input_ids[~replaced], cap[~replaced]):
        out.append(f"{int((input_ids != cap)[~replaced].sum())} unreplaced slots differ from the caption")
    _, _, lp = roll_in(case, p, u, ids=input_ids)
    m = replaced & want
    lo, hi = interval_excess(lp, input_ids.clamp(0, lp.shape[2] - 1), u[1])
    d = d_bound(case)
    bad = m & ~((lo <= d) & (hi < d))
    if bad.any():
        out.append(f"{int(bad.sum())} of {int(m.sum())} replaced slots outside the interval rule (worst {max(lo[m].max(), hi[m].max()):.2e}, d {d:.2e})")
    return out


FLOOR_SEEDS = range(100, 108)


def floor(case):
    """CDF distance between fp32 and float64 arithmetic of the restatement, teacher-forced on the float64 oracle's own mixed ids.
    The bf16 cases differ wherever a stored value rounds the other way, a rare event that moves a whole row: with the few dozen
    replaced slots of one roll-in the maximum would say more about luck than about the arithmetic, so it is taken over every
    slot a step produces logits for and over the roll-ins of FLOOR_SEEDS (other uniforms, other mixed prefixes)."""
    _, _, _, lens, _ = inputs(case)
    worst = 0.0
    for seed in FLOOR_SEEDS:
        u = uniforms(case, seed)
        ids, _, lp64 = roll_in(case, u=u)
        _, _, lp32 = roll_in(case, u=u, ids=ids, dt=torch.float32)
        cdf32 = torch.from_numpy(np.cumsum(lp32.exp().numpy(), axis=2, dtype=np.float32)).double()
        m = torch.from_numpy(valid_slots(family(case), lens, ids.shape[1]))
        worst = max(worst, float((cdf32 - lp64.exp().cumsum(2)).abs()[m].max()))
    return worst


# ---- the loss with input ids apart from the targets ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def random_ids(case):
    """X (B, T) int64 in [4, V): differs from the caption (almost) everywhere and never holds <start> = 1 or <end> = 2, which
    the targets do hold, so their embedding rows must get a gradient of exactly zero."""
    _, _, cap, _, _ = inputs(case)
    V = inputs(case)[0]["linear.bias"].shape[0]
    x = torch.randint(4, V, tuple(cap.shape), generator=torch.Generator().manual_seed(41 + len(case)))
    return torch.where(x == cap, (x - 4 + 1) % (V - 4) + 4, x)


def target_only_tokens(case):
    """Tokens that occur in the packed targets but nowhere in X."""
    _, _, cap, lens, _ = inputs(case)
    return sorted(set(R.pack_rows(cap, lens).tolist()) - set(random_ids(case).reshape(-1).tolist()))


@functools.lru_cache(maxsize=None)
def weights(case):
    cap = inputs(case)[2]
    g = torch.Generator().manual_seed(19 + len(case))
    return torch.rand(cap.shape[0], generator=g) * 2 - 1, torch.rand(tuple(cap.shape), generator=g) * 2 - 1


def packed_weights(case):
    sw, tw = weights(case)
    return R.pack_rows(sw.double()[:, None] * tw.double(), inputs(case)[3])


def _unit_logits(case, po, fo, X, lens):
    """A double nn.GRU / nn.LSTM on [feat ; embeddings(X)] over the packed sequence, then `linear`: (N_tok, V)."""
    _, cell, _, E, H, V, L, _ = CASES[case]
    unit = (nn.GRU if cell == "gru" else nn.LSTM)(E, H, L, batch_first=True).double()
    names = [n for n, _ in unit.named_parameters()]
    raw = torch.cat((fo.unsqueeze(1), po["embeddings.weight"][X]), 1)
    packed = nn.utils.rnn.pack_padded_sequence(raw, lens, batch_first=True)
    out = torch.func.functional_call(unit, {n: po["unit." + n] for n in names}, (packed,))[0]
    return out.data @ po["linear.weight"].t() + po["linear.bias"]


def _site_masks(ntok, E, H, L, step=0):
    (p_in, p_layer, p_out), seed = DROPOUT["p"], DROPOUT["seed"]
    out = {D.SITE_INPUT: D.multiplier(seed, step, D.SITE_INPUT, ntok, E, p_in)}
    for l in range(L):
        out[l] = D.multiplier(seed, step, l, ntok, H, p_out if l == L - 1 else p_layer)
    return out


def _walk_logits(case, po, fo, X, lens, masks):
    """The layer walk of tests/_dropout_cases.py (rnn_loss) on [feat ; embeddings(X)] with the given masks."""
    _, cell, _, E, H, V, L, B = CASES[case]
    bs = R.batch_sizes(lens)
    off = np.concatenate([[0], np.cumsum(bs)])
    rows = R.pack_rows(torch.cat((fo.unsqueeze(1), po["embeddings.weight"][X]), 1), lens) * masks[D.SITE_INPUT]
    for l in range(L):
        w_ih, w_hh, b_ih, b_hh = R._layer_w(po, l)
        h, c, out = rows.new_zeros(B, H), rows.new_zeros(B, H), []
        for t, b in enumerate(bs):
            x = rows[off[t]:off[t + 1]]
            if cell == "gru":
                hn = R.gru_cell(x, h[:b], w_ih, w_hh, b_ih, b_hh)
            else:
                hn, cn = R.lstm_cell(x, h[:b], c[:b], w_ih, w_hh, b_ih, b_hh)
                c = torch.cat([cn, c[b:]], 0)
            h = torch.cat([hn, h[b:]], 0)
            out.append(hn)
        rows = torch.cat(out, 0) * masks[l]
    return rows @ po["linear.weight"].t() + po["linear.bias"]


LOSS_FAULTS = ("emb_grad_by_caption", "targets_from_ids")


class _Lookup(torch.autograd.Function):
    """emb[X] whose gradient scatters to the rows of `scatter` (the seeded fault: the caption's, not X's)."""

    @staticmethod
    def forward(ctx, emb, X, scatter):
        ctx.save_for_backward(scatter)
        ctx.shape = emb.shape
        return emb[X]

    @staticmethod
    def backward(ctx, g):
        (scatter,) = ctx.saved_tensors
        out = g.new_zeros(ctx.shape)
        out.index_add_(0, scatter.reshape(-1), g.reshape(-1, g.shape[-1]))
        return out, None, None


@functools.lru_cache(maxsize=None)
def loss_reference(case, variant, fault=None):
    """{'loss', 'g', 'gp', 'gm'} of loss(input_ids = X) in float64 (the layout of tests/_weighted_loss_cases.oracle_grads).
    variant 'plain': unweighted, unsmoothed; 'w_ls': signed sequence and token weights and label smoothing; 'dropout' (plain
    decoders): the masks of DROPOUT at step 0.  fault: one of LOSS_FAULTS, expressed in the oracle."""
    params, feat, cap, lens, alpha_c = inputs(case)
    X = random_ids(case)
    attn = family(case) == "attn"
    po = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    fo = feat.double().clone().requires_grad_(not attn)
    alphas = None
    if fault == "emb_grad_by_caption":
        po_in = dict(po)
        emb = po["embeddings.weight"]

        class _E:                       # emb[X] with the faulty scatter, for the one indexing expression the oracles use
            def __getitem__(self, idx):
                return _Lookup.apply(emb, idx, cap)
        po_in["embeddings.weight"] = _E()
    else:
        po_in = po
    if attn:
        logits, alphas = R.attn_forward(po_in, fo, X, lens, cell_of(case))
    elif variant == "dropout":
        _, _, _, E, H, V, L, _ = CASES[case]
        logits = _walk_logits(case, po_in, fo, X, lens, _site_masks(sum(lens), E, H, L))
    else:
        logits = _unit_logits(case, po_in, fo, X, lens)
    target = R.pack_rows(X if fault == "targets_from_ids" else cap, lens)
    n = target.shape[0]
    w = packed_weights(case) if variant == "w_ls" else torch.ones(n, dtype=torch.float64)
    eps = LABEL_SMOOTHING[dtype_name(case)] if variant == "w_ls" else 0.0
    leaves = dict(po)
    if not attn:
        leaves["feat"] = fo
    out = {}
    for name, wk in (("g", w), ("gp", w.clamp(min=0)), ("gm", (-w).clamp(min=0))):
        loss = S.smoothed_loss(logits, alphas, target, wk, alpha_c, eps)
        gs = torch.autograd.grad(loss, list(leaves.values()), retain_graph=True, allow_unused=True)
        out[name] = {k: (torch.zeros_like(v) if g is None else g) for (k, v), g in zip(leaves.items(), gs)}
        if name == "g":
            out["loss"] = loss.item()
    out["mean_abs_w"] = w.abs().mean().item()
    return out


def loss_bound(case, ref):
    """|loss - oracle|: 2e-2 (bf16) / 1e-4 (fp32) times mean|w| of the run, + 3e-5 for the attention decoder's unweighted term."""
    if dtype_name(case) == "bf16":
        return 2e-2 * max(ref["mean_abs_w"], 1e-3)
    return 1e-4 * max(ref["mean_abs_w"], 1e-3) + (3e-5 if family(case) == "attn" else 0.0)


grad_scale = W.grad_scale
assert_grads_within_linear_bound = W.assert_grads_within_linear_bound


def grad_violations(got, ref, tol):
    """The parameters whose gradient lies outside the linear-form bound (what assert_grads_within_linear_bound asserts)."""
    bad = []
    for k, g in got.items():
        if k in ZERO_GRADS:
            continue
        if (g.double() - ref["g"][k]).abs().max().item() > tol * grad_scale(ref, k):
            bad.append(k)
    return bad


if __name__ == "__main__":
    torch.set_num_threads(8)
    for case in CASES:
        ids, rep, lp = oracle_roll_in(case)
        ptok = lp.gather(2, ids[..., None]).squeeze(2).exp()[rep]
        print(f"    {case!r}: {floor(case):.2e},   # replaced {int(rep.sum())}, p(token) < 0.5 for {float((ptok < 0.5).double().mean()):.2f}", flush=True)
