"""Nucleus (top-p) sampling on the device (st_sample_rows_topp, st_rnn_sample_topp, st_attn_sample_topp; sample(.., top_p=))
against the float64 oracle and the judge of tests/_nucleus_cases.py (the rule and the judge are stated there).

A  st_sample_rows_topp on the 44 rows of tests/test_gpu_sample.py::rows_inputs, each with its own u, u = 0 and u -> 1 (the
   two added copies draw the first and the last kept index and, with logp, pin the kept set from outside); a boundary-tie
   row; the off switch top_p = 1 against st_sample_rows, bit for bit
B  the kernel's two routes over memory    C  small rows    D  the plain decoders    E  the attention decoders    F  the API

Bounds.  None comes from the kernel.  A to C: d is 4 x the largest distance between a sequential float32 evaluation (the
cumulative sum in the rule's descending order, the CDF in index order over the kept set) and the float64 one on the case's
own random rows (the 37 of rows_inputs, the 11 of route_inputs; the added rows are held to the same bound, as in
tests/test_gpu_sample.py), b is 4 x the fp32-against-float64 distance of the kept set's log-probabilities;
`python -m tests.test_gpu_nucleus` (CPU only) prints them.  D and E: d and b are tests/test_gpu_sample.py::bounds of the same
decoder case.  After the "#": the kernel's worst on the MI355X, how far u and logp lie outside the oracle's own range
(negative: inside it).

The power of these inputs and of the judge (nucleus sizes, the width of the judged range, six seeded faults) is asserted
from the oracle alone in tests/test_nucleus_inputs.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _nucleus_cases as N
from tests import test_gpu_sample as GS
from tests import test_sample_inputs as I
from tests.test_sample_inputs import END, START, T

pytestmark = pytest.mark.gpu

ROWS_V = GS.ROWS_V

# (temperature, top_k, top_p): (floor of d, floor of b); the bounds are 4 x these
A_FLOOR = {
    (1.0, 0, 0.9): (6.50e-06, 6.15e-07),                   # u 0.0 (on the range's edge at u = 0), logp 5.1e-07
    (0.7, 0, 0.5): (1.08e-05, 7.12e-07),                   # 1.9e-14, 1.8e-07
    (1.3, 0, 0.95): (3.40e-06, 1.05e-06),                  # 0.0, 8.0e-07
    (3.0, 0, 0.9): (2.25e-06, 1.02e-06),                   # 0.0, 1.0e-06
    (1.0, 32, 0.8): (2.38e-07, 2.56e-07),                  # 0.0, 2.5e-07
    (1.0, 5, 0.5): (2.38e-07, 8.03e-08),                   # 0.0, 8.2e-08
    (1.0, 0, 1e-06): (6.50e-06, 0.00e+00),                 # 0.0, 5.6e-17 (the float64 oracle's own rounding)
}
# the boundary-tie row is an added row: held to the floor of the 37 random rows at its own (1.0, 0, 0.7)
TIE_FLOOR = (6.50e-06, 4.07e-07)                           # 0.0, 2.9e-09
ROUTE_FLOOR = {                                              # (V, top_k) at top_p = 0.9
    (5003, 0): (5.66e-06, 4.19e-07),                       # -6.0e-08, 3.1e-07
    (5003, 5): (1.19e-07, 9.90e-08),                       # -6.0e-08, 2.5e-07
    (10243, 0): (9.77e-06, 6.13e-07),                      # -6.0e-08, 3.9e-07
    (10243, 5): (1.19e-07, 1.53e-07),                      # -6.0e-08, 1.1e-07
}
SMALL_FLOOR = {                                              # V at top_p = 0.7
    1: (0.00e+00, 0.00e+00),                               # -1.4e-01, 0.0
    7: (7.88e-08, 1.04e-07),                               # -2.6e-02, 1.0e-07
    300: (8.34e-07, 1.89e-07),                             # -5.2e-03, 1.6e-07
}
SMALL_P = 0.7


def _bound(floor):
    return 4 * floor[0], 4 * floor[1]


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _topp_rows(logits, u, fin, inv_t, k, top_p, end_id, V, stride=3, t=1):
    from showtell_amd._lib import check, lib
    n = logits.shape[0]
    logits, u, fin = logits.cuda(), u.cuda(), fin.clone().cuda()
    ids = torch.full((n, stride), -7, device="cuda", dtype=torch.long)
    logp = torch.full((n, stride), 7.0, device="cuda")
    cur = torch.full((n,), -7, device="cuda", dtype=torch.long)
    check(lib().st_sample_rows_topp(_ptr(logits), logits.stride(0), n, V, _ptr(u), 1, float(inv_t), int(k), float(top_p), int(end_id),
                                    _ptr(fin), _ptr(ids), _ptr(logp), stride, t, _ptr(cur), _stream()), "st_sample_rows_topp")
    torch.cuda.synchronize()
    ids, logp = ids.cpu(), logp.cpu()
    assert (ids[:, 0] == -7).all() and (ids[:, 2] == -7).all() and (logp[:, 0] == 7).all() and (logp[:, 2] == 7).all()
    return ids[:, 1], logp[:, 1], cur.cpu(), fin.cpu()


def _judge_rows(tag, logits, u, fin0, temperature, k, top_p, V, floor):
    """one launch, every live row judged; returns (tok, logp, the judge's dict, (d, b))"""
    rows = logits[:, :V]
    inv_t = I.inv_temperature(temperature)
    z = N.scaled(rows, inv_t)
    d, b = _bound(floor)
    end_id = int(N.oracle_draw(z[:1], k, top_p, u[:1])[0])   # what the oracle itself draws for row 0: the flag is exercised
    tok, logp, cur, fin = _topp_rows(logits, u, fin0, inv_t, k, top_p, end_id, V)
    live = fin0 == 0
    assert torch.equal(cur, tok) and ((tok >= 0) & (tok < V)).all()
    assert (tok[~live] == 0).all() and (logp[~live] == 0).all() and (fin[~live] == 1).all()
    j = N.judge(z, k, top_p, tok, logp, u, d, b)
    print(N.measure_line(tag, j, live, d, b))
    assert j["inside"][live].all(), "a token outside the widest nucleus"
    assert j["ok"][live].all(), tag
    assert torch.equal(fin[live] == 1, tok[live] == end_id), "finished exactly when the token is <end>"
    assert tok[0] == end_id
    return tok, logp, j, (d, b)


# ====================================================================================================================
# A: st_sample_rows_topp
# ====================================================================================================================

@pytest.mark.parametrize("temperature,k,top_p", N.A_CASES)
def test_nucleus_rows_against_float64_on_the_same_logits(temperature, k, top_p):
    logits, u, fin0, names, n = N.a_inputs()
    tok, logp, j, (d, b) = _judge_rows(f"rows temperature {temperature} top_k {k} top_p {top_p}", logits, u, fin0, temperature, k, top_p,
                                       ROWS_V, A_FLOOR[(temperature, k, top_p)])
    live = fin0 == 0
    for r in (names["single"], names["single"] + n, names["single"] + 2 * n):
        assert tok[r] == GS.SINGLE and logp[r] == 0
    if top_p == 1e-6:                                        # a nucleus of one: the first-index arg-max, exactly
        assert torch.equal(tok[live], logits[:, :ROWS_V][live].max(1)[1]) and (logp[live] == 0).all()
    if (temperature, k, top_p) == (0.7, 0, 0.5):             # the constant row keeps indices 0 .. 2501
        c = names["const"]
        assert tok[c + n] == 0 and tok[c + 2 * n] == 2501
        assert (logp[[c, c + n, c + 2 * n]].double() + np.log(2502.0)).abs().max() <= b


def test_nucleus_splits_a_tie_at_the_boundary_by_the_lower_index():
    """-inf everywhere but log 0.4 at 4000 and log 0.2 at 100, 2000, 3000; at top_p = 0.7 the nucleus is {4000, 100, 2000}, with a
    margin of 0.1 either side.  A kernel that split the tie by the higher index would draw 2000 at u = 0."""
    logits, u, fin0 = N.tie_inputs()
    tok, logp, j, (d, b) = _judge_rows("boundary tie", logits, u, fin0, 1.0, 0, N.TIE_P, ROWS_V, TIE_FLOOR)
    assert (j["m_lo"] == 3).all() and (j["m_hi"] == 3).all()
    assert tok[1] == 100 and tok[2] == 4000
    assert abs(float(logp[1]) - np.log(0.2 / 0.8)) <= b + 1e-7      # log 0.2 and log 0.4 as fp32 logits: 6e-8 each


@pytest.mark.parametrize("k", [0, 5])
def test_top_p_of_one_is_the_parent_launch_bit_for_bit(k):
    logits, u, fin0, names, n = N.a_inputs()
    lp, _ = GS.rows_oracle(logits[:, :ROWS_V], 1.0, k)
    end_id = int((lp[0].exp().cumsum(0) <= u[0].double()).sum().clamp(max=ROWS_V - 1))
    new = _topp_rows(logits, u, fin0, 1.0, k, 1.0, end_id, ROWS_V)
    ids, logp, cur, fin = GS._sample_rows(logits.cuda(), u.cuda(), fin0.clone().cuda(), 1.0, k, end_id)
    assert torch.equal(new[0], ids[:, 1]) and torch.equal(new[1], logp[:, 1]) and torch.equal(new[2], cur) and torch.equal(new[3], fin)
    assert new[0][0] == end_id and new[3][0] == 1


# ====================================================================================================================
# B: the routes over memory    C: small rows
# ====================================================================================================================

@pytest.mark.parametrize("V,ld", N.ROUTES)
@pytest.mark.parametrize("k", [0, 5])
def test_nucleus_routes_over_memory(V, ld, k):
    """(5003, 5003): rows that are not 16-byte aligned, scalar loads; (10243, 10244): more than 256 x 40 entries, 16-byte loads.
    The constant row (11, and 12 with u -> 1) keeps its first ceil(0.9 V) indices."""
    logits, u, fin0 = N.route_rows(V, ld)
    tok, logp, j, _ = _judge_rows(f"route V={V} ld={ld} top_k {k} top_p 0.9", logits, u, fin0, 1.0, k, 0.9, V, ROUTE_FLOOR[(V, k)])
    if k == 0:
        assert tok[12] == {5003: 4503, 10243: 9219}[V] - 1
    else:
        assert tok[11] < k and tok[12] == k - 1              # 5 x 0.2: c_excl = 0.8 < 0.9 keeps all five


@pytest.mark.parametrize("V", [1, 7, 300])
def test_nucleus_small_rows(V):
    """V = 300: most threads own an empty range"""
    logits, u, fin0 = N.small_rows(V)
    tok, logp, j, _ = _judge_rows(f"small V={V} top_p {SMALL_P}", logits, u, fin0, 1.0, 0, SMALL_P, V, SMALL_FLOOR[V])
    if V == 1:
        assert (tok == 0).all() and (logp == 0).all()


# ====================================================================================================================
# D, E: the decoders
# ====================================================================================================================

def _check_decoder(kind, cell, dtype, shape, k, top_p, out, tag):
    Bn, S = shape
    n = Bn * S
    storage = dtype == torch.bfloat16
    ids, logp, lengths = (x.cpu() for x in out[:3])
    assert ids.shape == logp.shape == (Bn, S, T) and lengths.shape == (Bn, S)
    assert ids.dtype == torch.long and logp.dtype == torch.float32 and lengths.dtype == torch.long
    ids, logp, lengths = ids.view(n, T), logp.view(n, T), lengths.view(n)
    assert ((ids >= 0) & (ids < I.V)).all()
    u = I.uniforms(Bn, S).view(n, T)
    lp, alphas = GS._walk(kind, cell, False, shape, 1.0, storage, ids)       # full-vocabulary log-probabilities along the GPU's ids
    m = I.checked_mask(ids)
    assert (ids[~m] == 0).all() and (logp[~m] == 0).all()
    first = torch.where((ids == END).any(1), (ids == END).long().argmax(1) + 1, torch.full((n,), T))
    assert torch.equal(lengths, m.sum(1)) and torch.equal(lengths, first)
    assert (logp <= 0).all()
    d, b, _ = GS.bounds(kind, cell, storage, 1.0, shape, False)
    j = N.judge_decoder(lp, k, top_p, ids, logp, u, d, b)
    print(N.measure_line(tag, j, m, d, b) + f"; pairs {int(m.sum())}, rows ended {int((lengths < T).sum())} of {n}")
    assert int(m.sum()) == int(lengths.sum())                # no (row, step) up to the first <end> is excluded
    assert j["ok"][m].all(), tag
    return m, alphas


# The kernels' worst on the MI355X against bounds(..) of tests/test_gpu_sample.py (u outside the oracle's range, logp outside it):
#   plain gru bf16 0.9: 1.8e-04 of d 4.0e-02, 2.0e-02 of b 2.3e-01; 0.5: -2.3e-04, 2.4e-02; top_k 20, 0.9: -2.3e-04, 2.6e-02
#   plain gru fp32 0.9: -9.4e-06 of d 1.7e-05, 1.4e-05 of b 5.4e-05; 0.5: -1.2e-05, 1.1e-05
#   plain lstm bf16 0.9: -2.7e-05 of d 5.3e-02, 3.5e-02 of b 2.7e-01; 0.5: 1.8e-03, 3.6e-02
#   plain lstm fp32 0.9: -1.6e-06 of d 1.7e-05, 1.6e-05 of b 5.1e-05; 0.5: -5.5e-05, 1.0e-05
#   attention gru bf16 0.9: -8.5e-06 of d 3.1e-02, 2.2e-02 of b 1.4e-01, alpha 1.4e-05 of 4.6e-05
#   attention lstm bf16 0.9: -2.3e-04 of d 4.6e-02, 3.1e-02 of b 2.0e-01, alpha 4.2e-06 of 1.7e-05
PLAIN = [(cell, dtype, 0, p) for cell in ("gru", "lstm") for dtype in (torch.bfloat16, torch.float32) for p in (0.9, 0.5)] \
    + [("gru", torch.bfloat16, 20, 0.9)]


@pytest.mark.parametrize("cell,dtype,k,top_p", PLAIN)
def test_plain_nucleus_samples_follow_the_storage_oracle(cell, dtype, k, top_p):
    shape = (23, 11)
    m = GS._model("plain", cell, False, dtype)
    out = m.sample(I.features("plain", 23).cuda(), 11, 1.0, k, T, END, uniforms=I.uniforms(23, 11).cuda(), top_p=top_p)
    _check_decoder("plain", cell, dtype, shape, k, top_p, out, f"plain {cell} {dtype} top_k {k} top_p {top_p}")


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_attention_nucleus_samples_follow_the_storage_oracle(cell):
    shape, dtype, P = (24, 3), torch.bfloat16, I.ATTN["P"]
    m = GS._model("attn", cell, False, dtype)
    f, u = I.features("attn", 24).cuda(), I.uniforms(24, 3).cuda()
    out = m.sample(f, 3, 1.0, 0, T, START, END, uniforms=u, return_alphas=True, top_p=0.9)
    assert out[3].shape == (24, 3, T, P) and out[3].dtype == torch.float32
    tag = f"attention {cell} top_p 0.9"
    msk, ref = _check_decoder("attn", cell, dtype, shape, 0, 0.9, out, tag)
    got = out[3].cpu().view(72, T, P).double()[msk]
    bound = GS.bounds("attn", cell, True, 1.0, shape, False)[2]
    print(f"MEASURE {tag}: alpha max |d| {(got - ref.double()[msk]).abs().max():.2e} (bound {bound:.2e})")
    assert (got >= 0).all() and ((got - ref.double()[msk]).abs() <= bound).all()
    assert ((got.sum(1) - 1).abs() <= GS.ALPHA_SUM).all()
    again = m.sample(f, 3, 1.0, 0, T, START, END, uniforms=u, top_p=0.9)
    assert len(again) == 3 and all(torch.equal(a, b) for a, b in zip(again, out[:3]))


# ====================================================================================================================
# F: the API
# ====================================================================================================================

@pytest.mark.parametrize("kind", ["plain", "attn"])
def test_same_seed_same_tensors_and_top_p_one_is_the_call_without_it(kind):
    Bn, S = 7, 3
    m = GS._model(kind, "gru", True, torch.bfloat16)
    f = I.features(kind, Bn).cuda()
    outs = []
    for _ in range(2):
        g = torch.Generator(device="cuda")
        g.manual_seed(5)
        outs.append(m.sample(f, num_samples=S, temperature=0.9, top_k=20, generator=g, top_p=0.9))
    assert all(torch.equal(x, y) for x, y in zip(outs[0], outs[1]))
    u = I.uniforms(Bn, S).cuda()
    for k in (0, 20):
        a, b = m.sample(f, num_samples=S, top_k=k, uniforms=u), m.sample(f, num_samples=S, top_k=k, uniforms=u, top_p=1.0)
        assert len(a) == len(b) == 3 and all(torch.equal(x, y) for x, y in zip(a, b))
    c = m.sample(f, num_samples=S, uniforms=u, top_p=0.5)
    assert not torch.equal(a[0], c[0])                       # the nucleus changes the captions


def test_rnn_sample_topp_allocates_and_synchronises_nothing():
    """st_rnn_sample_topp on a side stream with preallocated buffers, recorded into a graph: a capture admits neither an
    allocation nor a synchronisation, and its replay gives the eager call's tensors."""
    from showtell_amd._lib import check, lib
    m = GS._model("plain", "gru", True, torch.bfloat16)
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
        check(lib().st_rnn_sample_topp(C.byref(prm), _ptr(feat), n, steps, _ptr(u), 1.0, 0, 0.9, END, _ptr(ws), nbytes, _ptr(ids), _ptr(logp),
                                       _stream()), "st_rnn_sample_topp")
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
# the floors: `python -m tests.test_gpu_nucleus` (CPU only)
# ====================================================================================================================

if __name__ == "__main__":
    torch.set_num_threads(8)
    logits, u, fin, names = GS.rows_inputs()
    for t, k, p in N.A_CASES:
        print("    (%r, %d, %r): (%.2e, %.2e)," % ((t, k, p) + N.floors(logits[:GS.ROWS_N, :ROWS_V], I.inv_temperature(t), k, p)), flush=True)
    print("TIE_FLOOR = (%.2e, %.2e)" % N.floors(logits[:GS.ROWS_N, :ROWS_V], 1.0, 0, N.TIE_P))
    for V, ld in N.ROUTES:
        for k in (0, 5):
            rl, _, rf = N.route_rows(V, ld)
            print("    (%d, %d): (%.2e, %.2e)," % ((V, k) + N.floors(rl[:11, :V], 1.0, k, 0.9)), flush=True)
    for V in (1, 7, 300):
        sl, _, sf = N.small_rows(V)
        print("    %d: (%.2e, %.2e)," % ((V,) + N.floors(sl[:, :V], 1.0, 0, SMALL_P)), flush=True)
