"""Inputs of the caption-sampling tests (tests/test_gpu_sample.py imports the builders and the oracle from here), and the
proof, from the float64 oracle alone, that these inputs can catch a fault.  Nothing here needs a GPU.

The oracle is oracle/restatement.py's teacher-forced storage restatement at W = 1 (tests/_beam_oracle.py's StepOracle:
`_cells_storage`, `rnn_beam_step_bf16_storage`, `attn_beam_init_bf16_storage`, `attn_beam_step_bf16_storage`) on bf16-representable
weights, in float64; `Oracle.run` either draws its own tokens from the uniforms (free running) or walks given tokens.

A default-scaled decoder is nearly uniform over the vocabulary: every row has the same CDF and no check of "the token
that u selects" could tell one row from another.  So the vocabulary projection and the cells' matrices (unit.weight_*) are
scaled (`SHARPEN`), and in the <end>-boosted variant <end>'s bias is raised so that rows end at different steps.  The
conditions asserted here, for every decoder case of the GPU file:

  unpeaked     at least half of the sampled tokens have probability below 0.5
  wrong row    for at least 80 % of the (row, step) pairs the oracle's token fails the interval rule when judged against
               the neighbouring row's CDF: the same sample of the NEXT image, row r + S (a kernel that read another row's
               logits, state or uniform would be caught; the S rows of one image share the feature and all of step 0)
  next row     the same against row r + 1, for S > 1 mostly another sample of the SAME image, over the steps >= 1 (step 0 of
               one image's rows is identical): at least 80 % as well (the oracle shows 0.81 to 0.97)
  <end>        (boosted variant) at least a quarter of the rows draw <end> before the last step, at least a quarter never
               draw it, and the first <end> falls on at least three distinct positions > 0

`python -m tests.test_sample_inputs` prints the figures of every case."""
import numpy as np
import pytest
import torch

from oracle import restatement as R
from tests._beam_oracle import StepOracle
from tests._util import _bf16

START, END = 1, 2
T = 25
# plain decoders
E = H = 128
V, L, B = 600, 3, 40
# attention decoders
ATTN = dict(E=128, H=128, V=600, L=2, F=256, A=128, P=49, B=24)

# Per temperature (the kernels multiply the logits by 1 / temperature: the x 25 of temperature 1 would at 0.7 leave fewer
# than half of the tokens below probability 0.5) -- lin: scale of linear.weight; rec: scale of the cells' matrices
# unit.weight_ih_l* and unit.weight_hh_l*; boost: added to linear.bias[<end>] in the boosted variant.  Chosen on the CPU so
# that the float64 oracle alone meets the conditions below.
SHARPEN = {
    ("plain", "gru"): {1.0: dict(lin=25.0, rec=2.0, boost=6.0), 0.7: dict(lin=18.0, rec=2.0, boost=4.2)},
    ("plain", "lstm"): {1.0: dict(lin=60.0, rec=3.0, boost=5.0), 0.7: dict(lin=42.0, rec=2.5, boost=3.0)},
    ("attn", "gru"): {1.0: dict(lin=20.0, rec=2.0, boost=10.0)},
    ("attn", "lstm"): {1.0: dict(lin=60.0, rec=2.5, boost=6.0)},
}
# (B, S) of the decoder cases
SHAPES = {"plain": ((40, 1), (23, 11)), "attn": ((24, 1), (24, 3))}
TEMPERATURES = {"plain": (1.0, 0.7), "attn": (1.0,)}

_CACHE = {}


def inv_temperature(temperature):
    """the fp32 value the kernels multiply by (ctypes rounds 1 / temperature to float)"""
    return float(np.float32(1.0 / float(temperature)))


def decoder_params(kind, cell, boost, temperature=1.0):
    """bf16-representable parameters of the case's decoder, sharpened for the temperature it is sampled at"""
    key = ("params", kind, cell, boost, temperature)
    if key not in _CACHE:
        if kind == "plain":
            p = R.init_decoder_params(E, H, V, L, cell, seed=9)
        else:
            a = ATTN
            p = R.init_decoder_params(a["E"], a["H"], a["V"], a["L"], cell, seed=9, attn=dict(F=a["F"], A=a["A"]))
        s = SHARPEN[(kind, cell)][temperature]
        p = {k: v.clone() for k, v in p.items()}
        p["linear.weight"] *= s["lin"]
        for k in p:
            if k.startswith("unit.weight"):
                p[k] *= s["rec"]
        if boost:
            p["linear.bias"][END] += s["boost"]
        _CACHE[key] = {k: _bf16(v) for k, v in p.items()}
    return _CACHE[key]


def features(kind, n):
    g = torch.Generator().manual_seed(9)
    if kind == "plain":
        return _bf16(torch.randn(n, E, generator=g))
    return _bf16(torch.randn(n, ATTN["F"], ATTN["P"], generator=g).abs())       # post-ReLU features are >= 0


def uniforms(n, S, steps=T):
    return torch.rand(n, S, steps, generator=torch.Generator().manual_seed(11))


class Oracle:
    """The storage oracle of one decoder on rows (image b, sample s) -> b * S + s, computed in `dt`."""

    def __init__(self, kind, cell, params, feat, S, storage=True, dt=torch.float64):
        self.kind, self.cell, self.storage = kind, cell, storage
        self.orc = StepOracle(kind, cell, params, feat.repeat_interleave(S, 0), 1, storage, dt)
        self.p, self.feat, self.n = self.orc.p, self.orc.feat, self.orc.B

    def run(self, u, temperature=1.0, ids=None, steps=T):
        """u (n, steps).  ids None: the oracle draws its own tokens (free running: the smallest v whose inclusive cumulative
        probability exceeds u; 0 after <end>); else it walks the given ids (n, steps), teacher-forced, its state never taken
        from anywhere else.  Returns (ids, logp (n, steps, V) = log_softmax(logits * inv_temperature) of every step, alphas
        (n, steps, P) or None)."""
        orc, n = self.orc, self.n
        it = inv_temperature(temperature)
        out_ids = torch.zeros(n, steps, dtype=torch.long)
        lps, als = [], []
        fin = torch.zeros(n, dtype=torch.bool)
        raw, state = orc.start()                                             # plain: step 0 is the feature from a zero state
        alpha = None
        if raw is None:
            raw, alpha, state = orc.step(torch.full((n, 1), START), state)
        for t in range(steps):
            lp = torch.log_softmax(raw * it, 1)
            lps.append(lp)
            als.append(alpha)
            if ids is None:
                cdf = lp.exp().cumsum(1)
                tok = (cdf <= u[:, t].to(cdf.dtype)[:, None]).sum(1).clamp(max=orc.V - 1)
                tok = torch.where(fin, torch.zeros_like(tok), tok)
            else:
                tok = ids[:, t]
            out_ids[:, t] = tok
            fin |= tok == END
            if t + 1 == steps:
                break
            raw, alpha, state = orc.step(tok.view(n, 1), state)
        return out_ids, torch.stack(lps, 1), (None if als[0] is None else torch.stack(als, 1))


def checked_mask(ids):
    """(row, step) pairs before and including the row's first <end>"""
    e = (ids == END).long()
    return (e.cumsum(1) - e) == 0


def interval_excess(lp, ids, u):
    """The interval rule c_lo - d <= u < c_hi + d of every (row, step): returns (c_lo - u, u - c_hi), both <= 0 inside the
    oracle's own interval.  lp (n, T, V) log-probabilities over the kept set (-inf outside), ids and u (n, T)."""
    p = lp.double().exp()
    c_hi = p.cumsum(2).gather(2, ids[..., None]).squeeze(2)
    c_lo = c_hi - p.gather(2, ids[..., None]).squeeze(2)
    u = u.double()
    return c_lo - u, u - c_hi


def interval_ok(lp, ids, u, d):
    lo, hi = interval_excess(lp, ids, u)
    return (lo <= d) & (hi < d)


def conditions(kind, cell, boost, shape, temperature, storage=True):
    """the figures of one decoder case from the float64 oracle's free-running sampling"""
    from tests.test_gpu_sample import bounds                # the bound the GPU test judges the interval rule with
    Bn, S = shape
    u = uniforms(Bn, S).view(Bn * S, T)
    ids, lp, _ = Oracle(kind, cell, decoder_params(kind, cell, boost, temperature), features(kind, Bn), S, storage).run(u, temperature)
    m = checked_mask(ids)
    p_tok = lp.gather(2, ids[..., None]).squeeze(2).exp()
    d = bounds(kind, cell, storage, temperature, shape, boost)[0]
    assert interval_ok(lp, ids, u, 0.0)[m].all()            # the oracle obeys its own rule exactly
    wrong = ~interval_ok(lp.roll(-S, 0), ids, u, d)         # row (b, s) judged against the distributions of row (b + 1, s)
    later = m.clone(); later[:, 0] = False                 # the S rows of an image share all of step 0
    wrong1 = ~interval_ok(lp.roll(-1, 0), ids, u, d)        # row r judged against row r + 1: for S > 1 mostly the same image
    is_end = ids == END
    first = torch.where(is_end.any(1), is_end.long().argmax(1), torch.full((Bn * S,), -1))
    return dict(unpeaked=float((p_tok[m] < 0.5).double().mean()), wrong_row=float(wrong[m].double().mean()),
                wrong_next=float(wrong1[later].double().mean()),
                early=float(((first >= 0) & (first < T - 1)).double().mean()), never=float((first < 0).double().mean()),
                positions=sorted({int(f) for f in first if f > 0}), pairs=int(m.sum()))


CASES = [(kind, cell, shape, t) for kind in ("plain", "attn") for cell in ("gru", "lstm") for shape in SHAPES[kind]
         for t in TEMPERATURES[kind]]


@pytest.mark.parametrize("kind,cell,shape,temperature", CASES)
def test_the_oracle_alone_meets_the_input_conditions(kind, cell, shape, temperature):
    for boost in (False, True):
        c = conditions(kind, cell, boost, shape, temperature)
        print(f"MEASURE {kind} {cell} (B, S)={shape} temperature {temperature} boost={boost}: {c}")
        assert c["unpeaked"] >= 0.5, c
        assert c["wrong_row"] >= 0.8, c
        assert c["wrong_next"] >= 0.8, c
        if boost:
            assert c["early"] >= 0.25 and c["never"] >= 0.25 and len(c["positions"]) >= 3, c


def _cpu_decoders():
    from showtell_amd.rnn import RNN
    from showtell_amd.rnn_attn import RNN_Attn
    a = ATTN
    return [(RNN(E, H, V, L), torch.zeros(3, E)),
            (RNN_Attn(a["E"], a["F"], a["A"], a["H"], a["V"], a["L"]), torch.zeros(3, a["F"], a["P"]))]


@pytest.mark.parametrize("which", [0, 1])
def test_argument_errors_are_raised_before_the_device_is_touched(which):
    """On CPU tensors: a ValueError, not the 'needs a HIP device' error that anything later would raise."""
    m, feat = _cpu_decoders()[which]
    for bad in (dict(temperature=0.0), dict(temperature=-1.0), dict(top_k=-1), dict(top_k=33), dict(num_samples=0),
                dict(uniforms=torch.zeros(3, 1, T - 1)), dict(uniforms=torch.zeros(3, 2, T)),
                dict(uniforms=torch.zeros(3, 1, T, dtype=torch.float64))):
        with pytest.raises(ValueError):
            m.sample(feat, **bad)
    small = type(m)(*((8, 8, 20, 1) if which == 0 else (8, 8, 8, 8, 20, 1)))
    with pytest.raises(ValueError):
        small.sample(feat, top_k=21)                        # top_k <= min(32, V)


if __name__ == "__main__":
    for case in CASES:
        for boost in (False, True):
            print("CONDITIONS", case, "boost", boost, conditions(case[0], case[1], boost, case[2], case[3]), flush=True)
