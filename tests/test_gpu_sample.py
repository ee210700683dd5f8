"""Caption sampling on the device (st_sample_rows, st_rnn_sample, st_attn_sample; RNN.sample, RNN_Attn.sample) against a
float64 oracle.  The kernels hold no random-number generator, the caller's uniforms decide every draw, so every check is
deterministic:

A  st_sample_rows alone against float64 on the SAME fp32 logits: the interval rule c_lo - d <= u < c_hi + d for the
   oracle's cumulative probability before / including the token, the token inside the kept set exactly, logp, the
   finished bytes, and the edge rows (constant, one finite entry, u = 0, u = nextafter(1, 0), a tie at the top_k
   boundary, rows finished on entry)
B  the plain decoders: the oracle (tests/test_sample_inputs.py: oracle/restatement.py at W = 1) walks the GPU's own ids,
   teacher-forced, its state never taken from the GPU, and judges every (row, step) before and including the first <end>
   by the interval rule and by |logp - oracle log p(token)|; after <end> tokens and logp are 0, lengths are exact
C  top_k at decoder level    D  the attention decoders, with the recorded attention maps    E  the API

Bounds.  None comes from the kernels.  A: 4x the largest distance between an fp32 evaluation (sequential float32
cumulative sum) and the float64 one of these same inputs.  B to D: 4x the distance between the SAME storage restatement in
fp32 and in float64 arithmetic, teacher-forced on the float64 oracle's free-running tokens, each case its own.  `python -m tests.test_gpu_sample` (CPU only) prints them all; the kernels' worst
measured values on the MI355X follow each constant after the "#".

A also runs the kernel's two other routes (rows longer than 256 x 40 entries, rows that are not 16-byte aligned).

Mutation check (injected once into a scratch build, not committed): st_sample_rows reading the NEXT row's uniform fails all
of A except top_k = 1 (which ignores u), every case of B and every case of D; C and E pass, as they must.

The power of the decoder cases to catch a fault (unpeaked distributions, the wrong-row fault, the spread of <end>) is
asserted from the oracle alone in tests/test_sample_inputs.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import test_sample_inputs as I
from tests.test_sample_inputs import END, START, T

pytestmark = pytest.mark.gpu

# ====================================================================================================================
# A: st_sample_rows
# ====================================================================================================================
ROWS_N, ROWS_V, ROWS_LD = 37, 5003, 5008
ROW_CASES = [(1.0, 0), (0.7, 0), (1.0, 5), (1.3, 32), (1.0, 1)]
# (d of the interval rule, logp): 4 x the fp32-against-float64 floor of the 37 random rows (`python -m tests.test_gpu_sample`
# prints them; the added rows are held to the same bound).  The two full-vocabulary values of d are DELIBERATELY not the
# printed ones: the script prints 5.88e-6 (temperature 1) and 7.09e-6 (0.7) -- a sequential float32 sum of 5003 terms, each
# addition rounded at the running sum's spacing, up to 6e-8: a random walk of 5003 such roundings is 2e-6 to 6e-6 -- and the
# feature was specified with 2.4e-7 and 2.9e-7.  The smaller, specified values are kept (the kernel sums hierarchically and
# meets them); do not raise them to the printed ones.
# After the "#": the kernel's worst on the MI355X (how far u lies inside or outside the oracle's interval, |d logp|).
ROWS_BOUND = {
    (1.0, 0): (4 * 2.4e-7, 4 * 2.04e-6),                    # inside the oracle's interval by 2.5e-8, 3.7e-7
    (0.7, 0): (4 * 2.9e-7, 4 * 4.09e-6),                    # inside by 6.5e-11, 8.9e-7
    (1.0, 5): (4 * 1.78e-7, 4 * 1.51e-7),                   # inside by 6.0e-8, 1.8e-7
    (1.3, 32): (4 * 2.38e-7, 4 * 5.55e-7),                  # inside by 6.0e-8, 3.2e-7
    (1.0, 1): (0.0, 0.0),                                   # one kept token: c_lo = 0, c_hi = 1, logp = 0, all exact; 0, 0
}
SINGLE = 1234                  # the one finite entry of its row


def rows_inputs():
    """(logits (n, ROWS_LD) fp32 with the padding columns poisoned, u (n), finished (n) uint8, names of the added rows)"""
    g = torch.Generator().manual_seed(3)
    base = torch.randn(ROWS_N, ROWS_V, generator=g) * 3
    u = torch.rand(ROWS_N, generator=g)
    extra = torch.randn(5, ROWS_V, generator=g) * 3          # u = 0, u -> 1, the tie row, two finished rows
    const = torch.full((1, ROWS_V), 1.25)
    single = torch.full((1, ROWS_V), -float("inf")); single[0, SINGLE] = 0.5
    tie = extra[2]
    at = torch.randperm(ROWS_V, generator=g)[:40]
    big = 20.0 - 0.25 * torch.arange(40.0)
    for k in (1, 5, 32):                                     # the k-th and the (k+1)-th largest are equal
        big[k] = big[k - 1]
    tie[at] = big
    rows = torch.cat([base, const, single, extra], 0)
    names = dict(const=ROWS_N, single=ROWS_N + 1, u0=ROWS_N + 2, u1=ROWS_N + 3, tie=ROWS_N + 4, fin=(ROWS_N + 5, ROWS_N + 6))
    uu = torch.cat([u, torch.tensor([0.5, 0.3, 0.0, float(np.nextafter(np.float32(1), np.float32(0))), 0.37, 0.2, 0.9])])
    n = rows.shape[0]
    logits = torch.full((n, ROWS_LD), 1e4)                   # never a value: a kernel that read the padding would pick it
    logits[:, :ROWS_V] = rows
    fin = torch.zeros(n, dtype=torch.uint8)
    fin[list(names["fin"])] = 1
    return logits, uu.float(), fin, names


def rows_oracle(rows, inv_t, k, dt=torch.float64):
    """(log-probabilities (n, V) in `dt` over the kept set, -inf outside; kept mask): the top k by value, the lowest index first
    among equal values"""
    keep = torch.ones_like(rows, dtype=torch.bool)
    if k:
        order = torch.sort(rows, dim=1, descending=True, stable=True).indices[:, :k]
        keep = torch.zeros_like(keep).scatter_(1, order, True)
    z = rows.to(dt) * torch.tensor(inv_t, dtype=dt)
    z = torch.where(keep, z, torch.full_like(z, -float("inf")))
    return torch.log_softmax(z, 1), keep


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _sample_rows(logits, u, fin, inv_t, k, end_id, stride=3, t=1, V=ROWS_V):
    from showtell_amd._lib import check, lib
    n = logits.shape[0]
    dev = logits.device
    ids = torch.full((n, stride), -7, device=dev, dtype=torch.long)
    logp = torch.full((n, stride), 7.0, device=dev)
    cur = torch.full((n,), -7, device=dev, dtype=torch.long)
    check(lib().st_sample_rows(_ptr(logits), logits.stride(0), n, V, _ptr(u), 1, float(inv_t), int(k), int(end_id), _ptr(fin),
                               _ptr(ids), _ptr(logp), stride, t, _ptr(cur), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
          "st_sample_rows")
    torch.cuda.synchronize()
    return ids.cpu(), logp.cpu(), cur.cpu(), fin.cpu()


@pytest.mark.parametrize("temperature,k", ROW_CASES)
def test_sample_rows_against_float64_on_the_same_logits(temperature, k):
    logits, u, fin0, names = rows_inputs()
    rows = logits[:, :ROWS_V]
    inv_t = I.inv_temperature(temperature)
    lp, keep = rows_oracle(rows, inv_t, k)
    live = fin0 == 0
    if k:
        # the tie row draws the LOWER index of the two equal logits at the top_k boundary: u is the middle of that token's
        # interval of the oracle's CDF, so a kernel that kept the higher index instead cannot return it
        r = names["tie"]
        top = torch.sort(rows[r], descending=True, stable=True).indices
        assert rows[r, top[k - 1]] == rows[r, top[k]] and top[k - 1] < top[k] and keep[r, top[k - 1]] and not keep[r, top[k]]
        p = lp[r].exp()
        c_hi = p.cumsum(0)[top[k - 1]]
        u[r] = float(c_hi - 0.5 * p[top[k - 1]])
        assert p[top[k - 1]] > 1e-5 and c_hi - p[top[k - 1]] < u[r].double() < c_hi       # the interval survives the fp32 u
    # <end> is what the oracle itself draws for row 0, so that the flag is exercised
    end_id = int((lp[0].exp().cumsum(0) <= u[0].double()).sum().clamp(max=ROWS_V - 1))
    ids, logp, cur, fin = _sample_rows(logits.cuda(), u.cuda(), fin0.clone().cuda(), inv_t, k, end_id)
    assert (ids[:, 0] == -7).all() and (ids[:, 2] == -7).all() and (logp[:, 0] == 7).all() and (logp[:, 2] == 7).all()
    tok = ids[:, 1]
    assert torch.equal(cur, tok) and ((tok >= 0) & (tok < ROWS_V)).all()
    # rows finished on entry
    for r in names["fin"]:
        assert tok[r] == 0 and logp[r, 1] == 0 and fin[r] == 1
    d, lp_bound = ROWS_BOUND[(temperature, k)]
    lo, hi = I.interval_excess(lp[:, None], tok[:, None], u[:, None])
    lo, hi = lo[:, 0][live], hi[:, 0][live]
    err = (logp[:, 1].double() - lp.gather(1, tok[:, None])[:, 0]).abs()[live]
    print(f"MEASURE rows temperature {temperature} top_k {k}: interval excess below {lo.max():.2e} above {hi.max():.2e} (d {d:.2e}); "
          f"|d logp| {err.max():.2e} (bound {lp_bound:.2e}); rows that drew <end>: {int((tok[live] == end_id).sum())}")
    assert keep.gather(1, tok[:, None])[:, 0][live].all(), "a token outside the kept set"
    assert (lo <= d).all() and (hi < d).all()
    assert (err <= lp_bound).all()
    assert torch.equal(fin[live] == 1, tok[live] == end_id), "finished exactly when the token is <end>"
    assert tok[0] == end_id
    # the added rows
    assert tok[names["single"]] == SINGLE and logp[names["single"], 1] == 0
    if k:
        assert tok[names["tie"]] == top[k - 1]               # the lower index of the tied pair, drawn
    if k == 1:
        assert torch.equal(tok[live], rows[live].max(1)[1]) and (logp[:, 1][live] == 0).all()       # the first-index arg-max


# Rows of more than 256 x 40 entries, and rows that are not 16-byte aligned, take the kernel's passes over memory (the cases
# above stay in registers): (V, ld) = (5003, 5003) reads with scalar loads, (10243, 10244) with 16-byte loads.  The last row
# is constant: with top_k = 5 more than 1024 candidates, so the selection by rounds.  Bounds as ROWS_BOUND, from the 11
# random rows of each case.
ROUTE_BOUND = {                                             # (V, top_k): (d, logp)
    (5003, 0): (4 * 3.13e-06, 4 * 1.86e-06),
    (5003, 5): (4 * 7.39e-08, 4 * 1.45e-07),
    (10243, 0): (4 * 9.12e-06, 4 * 2.22e-06),
    (10243, 5): (4 * 1.19e-07, 4 * 1.53e-07),
}


def route_inputs(V, ld):
    g = torch.Generator().manual_seed(4)
    rows = torch.randn(12, V, generator=g) * 3
    rows[11] = 0.75
    logits = torch.full((12, ld), 1e4)
    logits[:, :V] = rows
    return logits, torch.rand(12, generator=g), torch.zeros(12, dtype=torch.uint8)


@pytest.mark.parametrize("V,ld,k", [(5003, 5003, 0), (5003, 5003, 5), (10243, 10244, 0), (10243, 10244, 5)])
def test_sample_rows_routes_over_memory(V, ld, k):
    logits, u, fin0 = route_inputs(V, ld)
    rows = logits[:, :V]
    lp, keep = rows_oracle(rows, 1.0, k)
    end_id = int((lp[0].exp().cumsum(0) <= u[0].double()).sum().clamp(max=V - 1))
    ids, logp, cur, fin = _sample_rows(logits.cuda(), u.cuda(), fin0.cuda(), 1.0, k, end_id, V=V)
    tok = ids[:, 1]
    assert torch.equal(cur, tok) and ((tok >= 0) & (tok < V)).all()
    d, lp_bound = ROUTE_BOUND[(V, k)]
    lo, hi = I.interval_excess(lp[:, None], tok[:, None], u[:, None])
    err = (logp[:, 1].double() - lp.gather(1, tok[:, None])[:, 0]).abs()
    print(f"MEASURE rows V={V} ld={ld} top_k {k}: interval excess below {lo.max():.2e} above {hi.max():.2e} (d {d:.2e}); "
          f"|d logp| {err.max():.2e} (bound {lp_bound:.2e})")
    assert keep.gather(1, tok[:, None]).all(), "a token outside the kept set"
    assert (lo <= d).all() and (hi < d).all() and (err <= lp_bound).all()
    assert torch.equal(fin == 1, tok == end_id) and tok[0] == end_id
    if k:
        assert tok[11] < k                                   # a constant row keeps its first k indices


# ====================================================================================================================
# B to D: the decoders
# ====================================================================================================================
# FLOORS[(kind, cell, storage, temperature, (B, S), boost)] = (CDF, log-probability in nats, max |d alpha|): the distance between
# the storage restatement in fp32 and in float64 arithmetic on the case's own inputs; storage
# True: the bf16 kernels against the bf16-storage oracle; False: the fp32 kernels against the unrounded float64 oracle (only
# the order of the sums differs).  Every bound is 4 x its own case's floor (`bounds`).  After the "#": the kernels'
# worst on the MI355X: u beyond the oracle's own interval (negative: inside it), |d logp|, |d alpha|; |sum alpha - 1| <= 1.5e-7.
FLOORS = {
    ('plain', 'gru', True, 1.0, (40, 1), False): (7.18e-03, 2.08e-02, 0.00e+00),  # 7.4e-03, 2.6e-02
    ('plain', 'gru', True, 1.0, (40, 1), True): (5.44e-03, 1.92e-02, 0.00e+00),  # 5.6e-04, 1.3e-02
    ('plain', 'gru', True, 1.0, (23, 11), False): (9.98e-03, 5.68e-02, 0.00e+00),  # 3.2e-03, 5.0e-02
    ('plain', 'gru', True, 1.0, (23, 11), True): (9.79e-03, 4.09e-02, 0.00e+00),  # 1.0e-03, 4.5e-02
    ('plain', 'gru', True, 0.7, (40, 1), False): (8.17e-03, 2.57e-02, 0.00e+00),  # -2.4e-05, 3.2e-02
    ('plain', 'gru', True, 0.7, (40, 1), True): (3.28e-03, 1.17e-02, 0.00e+00),  # 9.5e-04, 1.3e-02
    ('plain', 'gru', True, 0.7, (23, 11), False): (1.27e-02, 5.07e-02, 0.00e+00),  # 1.4e-03, 4.5e-02
    ('plain', 'gru', True, 0.7, (23, 11), True): (1.04e-02, 4.00e-02, 0.00e+00),  # 3.0e-03, 3.9e-02
    ('plain', 'gru', False, 1.0, (40, 1), False): (3.66e-06, 9.66e-06, 0.00e+00),  # -2.1e-06, 1.0e-05
    ('plain', 'gru', False, 1.0, (40, 1), True): (3.77e-06, 1.01e-05, 0.00e+00),  # -3.1e-06, 1.0e-05
    ('plain', 'gru', False, 1.0, (23, 11), False): (4.12e-06, 1.36e-05, 0.00e+00),  # -7.8e-08, 1.2e-05
    ('plain', 'gru', False, 1.0, (23, 11), True): (4.24e-06, 1.32e-05, 0.00e+00),  # -3.7e-07, 1.1e-05
    ('plain', 'gru', False, 0.7, (40, 1), False): (3.32e-06, 9.44e-06, 0.00e+00),  # -7.6e-06, 1.3e-05
    ('plain', 'gru', False, 0.7, (40, 1), True): (2.80e-06, 1.42e-05, 0.00e+00),  # -7.2e-07, 7.1e-06
    ('plain', 'gru', False, 0.7, (23, 11), False): (3.60e-06, 1.24e-05, 0.00e+00),  # 2.6e-07, 1.1e-05
    ('plain', 'gru', False, 0.7, (23, 11), True): (4.12e-06, 1.10e-05, 0.00e+00),  # 1.9e-07, 1.1e-05
    ('plain', 'lstm', True, 1.0, (40, 1), False): (1.06e-02, 4.70e-02, 0.00e+00),  # 4.8e-03, 5.4e-02
    ('plain', 'lstm', True, 1.0, (40, 1), True): (1.18e-02, 2.00e-02, 0.00e+00),  # 4.6e-03, 3.7e-02
    ('plain', 'lstm', True, 1.0, (23, 11), False): (1.33e-02, 6.86e-02, 0.00e+00),  # 7.5e-03, 6.8e-02
    ('plain', 'lstm', True, 1.0, (23, 11), True): (1.17e-02, 4.23e-02, 0.00e+00),  # 3.9e-03, 4.2e-02
    ('plain', 'lstm', True, 0.7, (40, 1), False): (7.20e-03, 3.29e-02, 0.00e+00),  # 1.8e-03, 2.4e-02
    ('plain', 'lstm', True, 0.7, (40, 1), True): (6.56e-03, 2.30e-02, 0.00e+00),  # 3.0e-03, 2.4e-02
    ('plain', 'lstm', True, 0.7, (23, 11), False): (9.20e-03, 3.93e-02, 0.00e+00),  # 3.4e-03, 4.5e-02
    ('plain', 'lstm', True, 0.7, (23, 11), True): (8.85e-03, 3.04e-02, 0.00e+00),  # 6.5e-03, 3.3e-02
    ('plain', 'lstm', False, 1.0, (40, 1), False): (3.21e-06, 9.26e-06, 0.00e+00),  # -9.1e-06, 1.2e-05
    ('plain', 'lstm', False, 1.0, (40, 1), True): (3.78e-06, 8.79e-06, 0.00e+00),  # -3.3e-05, 1.4e-05
    ('plain', 'lstm', False, 1.0, (23, 11), False): (4.12e-06, 1.28e-05, 0.00e+00),  # -8.7e-08, 1.5e-05
    ('plain', 'lstm', False, 1.0, (23, 11), True): (3.58e-06, 1.33e-05, 0.00e+00),  # -3.8e-08, 1.3e-05
    ('plain', 'lstm', False, 0.7, (40, 1), False): (2.90e-06, 8.80e-06, 0.00e+00),  # -4.4e-07, 7.4e-06
    ('plain', 'lstm', False, 0.7, (40, 1), True): (2.64e-06, 5.93e-06, 0.00e+00),  # -6.6e-07, 6.9e-06
    ('plain', 'lstm', False, 0.7, (23, 11), False): (3.06e-06, 9.73e-06, 0.00e+00),  # -3.3e-08, 8.9e-06
    ('plain', 'lstm', False, 0.7, (23, 11), True): (2.51e-06, 8.30e-06, 0.00e+00),  # 2.6e-07, 9.1e-06
    ('attn', 'gru', True, 1.0, (24, 1), False): (7.82e-03, 3.54e-02, 9.42e-06),  # 9.9e-04, 2.6e-02, 8.0e-06
    ('attn', 'gru', True, 1.0, (24, 1), True): (8.27e-03, 3.41e-02, 9.00e-06),  # -3.9e-06, 2.0e-02, 8.0e-06
    ('attn', 'gru', True, 1.0, (24, 3), False): (7.70e-03, 3.43e-02, 1.16e-05),  # 1.6e-03, 4.0e-02, 9.3e-06
    ('attn', 'gru', True, 1.0, (24, 3), True): (8.61e-03, 4.98e-02, 1.26e-05),  # 4.9e-04, 2.9e-02, 9.3e-06
    ('attn', 'gru', False, 1.0, (24, 1), False): (2.89e-06, 9.76e-06, 6.42e-09),  # -2.5e-06, 6.3e-06, 7.4e-09
    ('attn', 'gru', False, 1.0, (24, 1), True): (3.54e-06, 9.65e-06, 6.69e-09),  # -3.6e-06, 1.1e-05, 6.5e-09
    ('attn', 'gru', False, 1.0, (24, 3), False): (2.96e-06, 1.08e-05, 6.80e-09),  # -3.4e-07, 7.9e-06, 6.1e-09
    ('attn', 'gru', False, 1.0, (24, 3), True): (2.36e-06, 9.61e-06, 6.28e-09),  # -1.6e-07, 9.7e-06, 6.1e-09
    ('attn', 'lstm', True, 1.0, (24, 1), False): (1.06e-02, 4.41e-02, 4.35e-06),  # 4.7e-03, 4.1e-02, 4.1e-06
    ('attn', 'lstm', True, 1.0, (24, 1), True): (1.12e-02, 4.10e-02, 4.11e-06),  # 1.6e-03, 4.1e-02, 4.1e-06
    ('attn', 'lstm', True, 1.0, (24, 3), False): (1.16e-02, 4.95e-02, 4.36e-06),  # 2.2e-03, 2.5e-02, 3.5e-06
    ('attn', 'lstm', True, 1.0, (24, 3), True): (9.36e-03, 4.95e-02, 4.12e-06),  # 2.2e-03, 3.2e-02, 4.1e-06
    ('attn', 'lstm', False, 1.0, (24, 1), False): (3.45e-06, 8.42e-06, 6.42e-09),  # 8.3e-08, 9.9e-06, 5.3e-09
    ('attn', 'lstm', False, 1.0, (24, 1), True): (3.00e-06, 1.17e-05, 6.42e-09),  # -1.8e-05, 1.0e-05, 5.3e-09
    ('attn', 'lstm', False, 1.0, (24, 3), False): (3.24e-06, 1.49e-05, 5.82e-09),  # -4.2e-07, 9.2e-06, 5.6e-09
    ('attn', 'lstm', False, 1.0, (24, 3), True): (3.62e-06, 1.30e-05, 6.06e-09),  # -3.3e-06, 8.7e-06, 5.6e-09
}


def bounds(kind, cell, storage, temperature, shape, boost):
    """(d of the interval rule, |d logp| in nats, max |d alpha|) of one decoder case: 4 x its own floor"""
    return tuple(4 * f for f in FLOORS[(kind, cell, storage, temperature, tuple(shape), boost)])


ALPHA_SUM = 1e-5            # |sum - 1| of an fp32 softmax over 49 entries: 49 roundings of 6e-8 and the division

_CACHE = {}


def _model(kind, cell, boost, dtype, temperature=1.0):
    key = (kind, cell, boost, dtype, temperature)
    if key not in _CACHE:
        params = I.decoder_params(kind, cell, boost, temperature)
        if kind == "plain":
            from tests.test_gpu_decoder_bench_shape import _decoder
            _CACHE[key] = _decoder(cell, params, dtype, I.E, I.H, I.V, I.L).eval()
        else:
            from tests.test_gpu_attention_beam import _make
            _CACHE[key] = _make(cell, {k: v.clone() for k, v in params.items()}, dtype)
    return _CACHE[key]


def _walk(kind, cell, boost, shape, temperature, storage, ids):
    """the oracle's log-probabilities (n, T, V) and attention maps along the given ids (shared by the checks of a case)"""
    Bn, S = shape
    orc = I.Oracle(kind, cell, I.decoder_params(kind, cell, boost, temperature), I.features(kind, Bn), S, storage)
    _, lp, alphas = orc.run(I.uniforms(Bn, S).view(Bn * S, T), temperature, ids=ids)
    return lp, alphas


def _check_sample(kind, cell, boost, shape, temperature, dtype, out, tag):
    Bn, S = shape
    n = Bn * S
    storage = dtype == torch.bfloat16
    ids, logp, lengths = (x.cpu() for x in out[:3])
    assert ids.shape == logp.shape == (Bn, S, T) and lengths.shape == (Bn, S)
    assert ids.dtype == torch.long and logp.dtype == torch.float32 and lengths.dtype == torch.long
    ids, logp, lengths = ids.view(n, T), logp.view(n, T), lengths.view(n)
    assert ((ids >= 0) & (ids < I.V)).all()
    u = I.uniforms(Bn, S).view(n, T)
    lp, alphas = _walk(kind, cell, boost, shape, temperature, storage, ids)
    m = I.checked_mask(ids)
    # after <end>: <pad>, logp 0; lengths count <end>, T without one
    assert (ids[~m] == 0).all() and (logp[~m] == 0).all()
    assert torch.equal(lengths, m.sum(1))
    first = torch.where((ids == END).any(1), (ids == END).long().argmax(1) + 1, torch.full((n,), T))
    assert torch.equal(lengths, first)
    d, nll, _ = bounds(kind, cell, storage, temperature, shape, boost)
    lo, hi = I.interval_excess(lp, ids, u)
    err = (logp.double() - lp.gather(2, ids[..., None]).squeeze(2)).abs()
    checked = int(m.sum())
    print(f"MEASURE {tag}: interval excess below {lo[m].max():.2e} above {hi[m].max():.2e} (d {d:.2e}); |d logp| {err[m].max():.2e} "
          f"(bound {nll:.2e}); pairs checked {checked} of {int(lengths.sum())}, rows ended {int((lengths < T).sum())} of {n}")
    assert checked == int(lengths.sum())                      # no (row, step) up to the first <end> is excluded
    assert (lo[m] <= d).all() and (hi[m] < d).all(), tag
    assert (err[m] <= nll).all(), tag
    return ids, logp, m, lp, alphas


PLAIN_CASES = [(cell, dtype, shape, t, boost) for cell in ("gru", "lstm") for dtype in (torch.bfloat16, torch.float32)
               for shape in I.SHAPES["plain"] for t in I.TEMPERATURES["plain"] for boost in (False, True)]


@pytest.mark.parametrize("cell,dtype,shape,temperature,boost", PLAIN_CASES)
def test_plain_samples_follow_the_storage_oracle(cell, dtype, shape, temperature, boost):
    """(23, 11): 253 rows, a last row tile of the cell GEMM that is not whole"""
    Bn, S = shape
    m = _model("plain", cell, boost, dtype, temperature)
    out = m.sample(I.features("plain", Bn).cuda(), S, temperature, 0, T, END, uniforms=I.uniforms(Bn, S).cuda())
    _check_sample("plain", cell, boost, shape, temperature, dtype, out, f"plain {cell} {dtype} (B, S)={shape} T={temperature} boost={boost}")


@pytest.mark.parametrize("k", [5, 1])
def test_top_k_at_decoder_level(k):
    shape, cell, boost, dtype = (40, 1), "gru", True, torch.bfloat16
    m = _model("plain", cell, boost, dtype)
    ids, logp, lengths = (x.cpu().view(40, -1) for x in
                          m.sample(I.features("plain", 40).cuda(), 1, 1.0, k, T, END, uniforms=I.uniforms(40, 1).cuda()))
    lp, _ = _walk("plain", cell, boost, shape, 1.0, True, ids)         # full-vocabulary log-probabilities along the GPU's ids
    msk = I.checked_mask(ids)
    nll = bounds("plain", cell, True, 1.0, shape, boost)[1]
    tok_lp = lp.gather(2, ids[..., None]).squeeze(2)
    kth = lp.topk(k, dim=2).values[..., -1]
    print(f"MEASURE top_k {k}: token below the oracle's k-th largest by at most {(kth - tok_lp)[msk].max():.2e} (bound {2 * nll:.2e}); "
          f"logp - full-vocabulary log p >= {(logp.double() - tok_lp)[msk].min():.2e}; pairs {int(msk.sum())}")
    assert (tok_lp[msk] >= kth[msk] - 2 * nll).all()                    # at temperature 1 logit differences are log p differences
    assert (logp[msk] <= 0).all()
    assert (logp.double()[msk] >= tok_lp[msk] - nll).all()              # truncation only raises a kept token's probability
    assert (ids[~msk] == 0).all() and (logp[~msk] == 0).all() and torch.equal(lengths.view(-1), msk.sum(1))
    if k == 1:
        assert (logp == 0).all()


ATTN_CASES = [(cell, dtype, shape, boost) for cell in ("gru", "lstm") for dtype in (torch.bfloat16, torch.float32)
              for shape in I.SHAPES["attn"] for boost in (False, True)]


@pytest.mark.parametrize("cell,dtype,shape,boost", ATTN_CASES)
def test_attention_samples_follow_the_storage_oracle(cell, dtype, shape, boost):
    Bn, S = shape
    P = I.ATTN["P"]
    m = _model("attn", cell, boost, dtype)
    f, u = I.features("attn", Bn).cuda(), I.uniforms(Bn, S).cuda()
    out = m.sample(f, S, 1.0, 0, T, START, END, uniforms=u, return_alphas=True)
    assert out[3].shape == (Bn, S, T, P) and out[3].dtype == torch.float32
    tag = f"attention {cell} {dtype} (B, S)={shape} boost={boost}"
    ids, logp, msk, lp, ref = _check_sample("attn", cell, boost, shape, 1.0, dtype, out, tag)
    got = out[3].cpu().view(Bn * S, T, P).double()[msk]
    ref = ref.double()[msk]
    bound = bounds("attn", cell, dtype == torch.bfloat16, 1.0, shape, boost)[2]
    print(f"MEASURE {tag}: alpha max |d| {(got - ref).abs().max():.2e} (bound {bound:.2e}), |sum - 1| {(got.sum(1) - 1).abs().max():.2e}")
    assert (got >= 0).all() and ((got - ref).abs() <= bound).all()
    assert ((got.sum(1) - 1).abs() <= ALPHA_SUM).all()
    # without the maps: the same three tensors
    again = m.sample(f, S, 1.0, 0, T, START, END, uniforms=u)
    assert len(again) == 3 and all(torch.equal(a, b) for a, b in zip(again, out[:3]))


# ====================================================================================================================
# E: the API
# ====================================================================================================================

@pytest.mark.parametrize("kind", ["plain", "attn"])
def test_same_seed_or_same_uniforms_give_the_same_tensors(kind):
    Bn, S = 7, 3
    m = _model(kind, "gru", True, torch.bfloat16)
    f = I.features(kind, Bn).cuda()
    outs = []
    for _ in range(2):
        g = torch.Generator(device="cuda")
        g.manual_seed(5)
        outs.append(m.sample(f, num_samples=S, temperature=0.9, top_k=20, generator=g))
    u = I.uniforms(Bn, S).cuda()
    outs += [m.sample(f, num_samples=S, uniforms=u) for _ in range(2)]
    for a, b in ((outs[0], outs[1]), (outs[2], outs[3])):
        assert len(a) == 3 and all(torch.equal(x, y) for x, y in zip(a, b))
    ids, logp, lengths = outs[0]
    assert ids.shape == logp.shape == (Bn, S, I.T) and lengths.shape == (Bn, S)
    assert ids.dtype == torch.long and logp.dtype == torch.float32 and lengths.dtype == torch.long and ids.is_cuda
    assert not torch.equal(outs[0][0], outs[2][0])           # other uniforms, other captions


def test_rnn_sample_allocates_and_synchronises_nothing():
    """st_rnn_sample on a side stream with preallocated buffers, recorded into a graph: a capture admits neither an allocation
    nor a synchronisation, and its replay gives the eager call's tensors."""
    from showtell_amd._lib import check, lib
    m = _model("plain", "gru", True, torch.bfloat16)
    n, steps = 19, 9
    prm, keep = m._c_params()
    feat = I.features("plain", n).cuda().bfloat16()
    u = I.uniforms(n, 1, steps).view(n, steps).cuda()
    nbytes = lib().st_rnn_sample_workspace_bytes(C.byref(prm), n)
    ws = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
    ids = torch.empty(n, steps, device="cuda", dtype=torch.long)
    logp = torch.empty(n, steps, device="cuda")
    s = torch.cuda.Stream()

    def call():
        check(lib().st_rnn_sample(C.byref(prm), _ptr(feat), n, steps, _ptr(u), 1.0, 0, END, _ptr(ws), nbytes, _ptr(ids), _ptr(logp),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)), "st_rnn_sample")
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    s.synchronize()
    eager = (ids.clone(), logp.clone())
    ids.fill_(-1); logp.fill_(-1)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(ids, eager[0]) and torch.equal(logp, eager[1])
    assert ((ids >= 0) & (ids < I.V)).all()


# ====================================================================================================================
# the floors: `python -m tests.test_gpu_sample` (CPU only)
# ====================================================================================================================

def _rows_floor(temperature, k, rows=None):
    if rows is None:
        rows = rows_inputs()[0][:ROWS_N, :ROWS_V]            # the random rows; the added rows are held to the same bound
    inv_t = I.inv_temperature(temperature)
    lp64, keep = rows_oracle(rows, inv_t, k)
    lp32, _ = rows_oracle(rows, inv_t, k, torch.float32)
    z32 = torch.where(keep, rows * torch.tensor(inv_t, dtype=torch.float32), torch.full_like(rows, -float("inf")))
    cdf32 = np.cumsum(torch.softmax(z32, 1).numpy(), axis=1, dtype=np.float32)       # sequential float32 sum
    cdf = float(np.abs(cdf32.astype(np.float64) - lp64.exp().cumsum(1).numpy()).max())
    ok = keep & torch.isfinite(lp64)
    return cdf, float((lp32.double() - lp64)[ok].abs().max())


def _decoder_floor(kind, cell, storage, temperature, shape, boost):
    Bn, S = shape
    params, feat, u = I.decoder_params(kind, cell, boost, temperature), I.features(kind, Bn), I.uniforms(Bn, S).view(Bn * S, T)
    ids, lp64, a64 = I.Oracle(kind, cell, params, feat, S, storage).run(u, temperature)
    _, lp32, a32 = I.Oracle(kind, cell, params, feat, S, storage, torch.float32).run(u, temperature, ids=ids)
    m = I.checked_mask(ids)
    cdf32 = torch.from_numpy(np.cumsum(lp32.exp().numpy(), axis=2, dtype=np.float32)).double()      # sequential float32 sum
    tok = ids[..., None]
    return (float((cdf32 - lp64.exp().cumsum(2)).abs()[m].max()),
            float((lp32.gather(2, tok).double() - lp64.gather(2, tok)).abs().squeeze(2)[m].max()),
            0.0 if a64 is None else float((a32.double() - a64).abs()[m].max()))


if __name__ == "__main__":
    torch.set_num_threads(8)
    for case in ROW_CASES:
        print("FLOOR rows", case, "cdf %.2e logp %.2e" % _rows_floor(*case), flush=True)
    for V, ld in ((5003, 5003), (10243, 10244)):
        for k in (0, 5):
            print("    (%d, %d): (4 * %.2e, 4 * %.2e)," % ((V, k) + _rows_floor(1.0, k, route_inputs(V, ld)[0][:11, :V])), flush=True)
    for kind in ("plain", "attn"):
        for cell in ("gru", "lstm"):
            for storage in (True, False):
                for t in I.TEMPERATURES[kind]:
                    for shape in I.SHAPES[kind]:
                        for boost in (False, True):
                            key = (kind, cell, storage, t, shape, boost)
                            print("    %r: (%.2e, %.2e, %.2e)," % ((key,) + _decoder_floor(*key)), flush=True)
