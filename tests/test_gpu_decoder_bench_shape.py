"""The bf16 decoder paths bench.py times, against a float64 oracle (oracle/restatement.py on bf16-representable weights).

A  rnn.loss() with the fused vocabulary cross entropy (csrc/vocab_ce.hip) at shapes where a workgroup walks several token
   tiles (mtiles > nsplit: the prefetch / tile_store / barrier sequence between tiles runs), and the launch chain beside it.
B  one bf16 configs[1] training step (encoder head on its split-K route -> 5-layer decoder -> fused cross entropy ->
   backward -> SGD with momentum), GRU and LSTM, full and ragged batches.
C  greedy decoding on the pipelined decoder (csrc/decode_pipe.hip) and on the launch chain against an oracle that keeps
   the kernels' bf16 storage (R.rnn_greedy_bf16_storage).
D  arg-max ties: every route must return torch.max's first maximal index.
E  st_rnn_greedy_last_route: the pipe really ran where it is asserted, and ineligible calls say so.

Bounds are set from bf16 storage rounding (2^-9 per stored value).  The worst errors measured on the MI355X are
written next to each bound.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import restatement as R
from tests._util import _bf16  # noqa: F401 (imported from here by other test modules)

pytestmark = pytest.mark.gpu

E = H = 512

# A / B bounds; measured worst on the MI355X (A: both cross-entropy routes, B: all four cases) after the "#"
LOSS_REL = 5e-3     # A 2.0e-5, B 2.2e-7
GRAD_L2 = 1e-2      # every gradient: A 5.3e-3, B 6.4e-3; SGD updates beyond one fp32 ulp 3.3e-3; BN1d batch statistics 2.3e-6
GRAD_MAX = 4e-2     # A 5.3e-3, B 6.6e-3; updates 5.3e-3; BN1d batch statistics 4.6e-6
ROW_L2 = 3e-2       # per sample d loss / d feat: A 6.9e-3, B 7.0e-3
BIAS_ELEM = 1e-2    # A linear.bias elementwise 2.1e-3 of max|ref|; B head Linear bias 5.0e-4 (grad), 7.3e-4 (update)


def _bf16_params(params):
    return {k: (_bf16(v) if v.is_floating_point() else v) for k, v in params.items()}


def _rel_l2(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return ((got - ref).norm() / (ref.norm() + 1e-300)).item()


def _rel_max(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-300)).item()


def _row_l2(got, ref):
    """worst per-row relative L2 error"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return ((got - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-300)).max().item()


def _decoder(cell, params, dtype, Ed, Hd, V, L):
    from showtell_amd.rnn import RNN
    from showtell_amd.rnn_lstm import RNN as RNN_LSTM
    m = (RNN if cell == "gru" else RNN_LSTM)(Ed, Hd, V, L, dtype=dtype)
    m.load_state_dict({k: v.clone() for k, v in params.items()})
    return m.cuda()


def _check_grads(got, ref, what, l2_bound=GRAD_L2, max_bound=GRAD_MAX):
    """relative L2 and relative max norm of one gradient tensor against the oracle"""
    l2, mx = _rel_l2(got, ref), _rel_max(got, ref)
    print(f"MEASURE {what}: rel_l2 {l2:.2e} rel_max {mx:.2e}")
    assert l2 < l2_bound and mx < max_bound, (what, l2, mx)
    return l2, mx


def _check_update(after, before, ref, what, l2_bound=GRAD_L2, max_bound=GRAD_MAX):
    """An updated fp32 parameter against the oracle's float64 update of the same starting values.  The parameter is
    stored in fp32, so each element may sit one fp32 ulp from the rounded oracle value however exact the gradient was
    (at lr 0.5 a step is ~1e-6 of the weight for some tensors: that ulp is several % of it).  What is left beyond that
    ulp is held to the gradient bounds, relative to the oracle's step."""
    ref32 = ref.float()
    ulp = (torch.nextafter(ref32.abs(), torch.tensor(math.inf)) - ref32.abs()).double()
    excess = ((after - ref32.double()).abs() - ulp).clamp_min(0)
    step = (ref - before).abs()
    l2, mx = (excess.norm() / step.norm()).item(), (excess.max() / step.max()).item()
    print(f"MEASURE {what}: beyond one fp32 ulp rel_l2 {l2:.2e} rel_max {mx:.2e}")
    assert l2 < l2_bound and mx < max_bound, (what, l2, mx)
    return l2, mx


def _captions(lens, V, seed):
    """zero-padded captions [1] + randint(4, V) + [2] for the given descending lengths (R.synthetic_captions' layout)"""
    rng = np.random.RandomState(seed)
    cap = np.zeros((len(lens), lens[0]), dtype=np.int64)
    for b, l in enumerate(lens):
        cap[b, 0] = 1
        cap[b, 1:l - 1] = rng.randint(4, V, size=l - 2)
        cap[b, l - 1] = 2
    return torch.from_numpy(cap), [int(l) for l in lens]


def _ragged_lens_100():
    """B = 100: every length 6..25 at least once, a run of equal lengths, sorted descending"""
    rng = np.random.RandomState(17)
    lens = list(range(6, 26)) + [int(v) for v in np.clip(np.rint(rng.normal(12.5, 4.0, size=80)), 6, 25)]
    lens = sorted(lens, reverse=True)
    assert min(lens) == 6 and max(lens) == 25 and max(lens.count(v) for v in set(lens)) >= 5
    return lens


# ====================================================================================================================
# A. fused vocabulary cross entropy past one token tile per workgroup
# ====================================================================================================================

def _vce_walk(ntok, V):
    """(mtiles, nsplit) exactly as csrc/vocab_ce.hip picks them: 32-token tiles, 128-entry tiles, vce_splits"""
    mtiles = (ntok + 31) // 32
    ntile = (V + 127) // 128
    nsplit = min(max(512 // ntile, 1), mtiles)
    return mtiles, nsplit


@pytest.mark.parametrize("cell,V,B,L,seed", [
    ("gru", 10000, 128, 5, 1),       # the benchmark shape: ntile 79, nsplit 6, 51 token tiles
    ("lstm", 4097, 64, 2, 2),        # ragged last entry tile (ntile 33, nsplit 15), 783 tokens (not a multiple of 32)
    ("gru", 70000, 16, 1, 3),        # ntile 547: nsplit 1, every workgroup walks every token tile
])
def test_fused_cross_entropy_multi_tile_walk_matches_fp64_oracle(cell, V, B, L, seed, monkeypatch):
    """Recurrent weights x2 and the vocabulary projection x6.  A default-initialised stack gives nearly the same top-layer
    row for every token and nearly uniform logits: a token tile computed from another tile's rows moved no bound (measured
    with the fault injected).  x2 / x6 make the rows token-dependent while the problem stays well conditioned: a float64
    relative perturbation of 2^-9 on every weight moves the gradients by <= 7e-3 in relative L2 here (at x5 by up to
    0.16, and the kernels then measured 6.6e-2: rounding amplification, not a kernel fault)."""
    params = R.init_decoder_params(E, H, V, L, cell, seed=seed)
    params["linear.weight"] *= 6.0
    for k in params:
        if k.startswith("unit.weight"):
            params[k] = params[k] * 2.0
    params = _bf16_params(params)
    cap, lens = R.synthetic_captions(B, V, seed=seed)
    ntok = sum(lens)
    mtiles, nsplit = _vce_walk(ntok, V)
    assert mtiles > nsplit, (mtiles, nsplit)               # several token tiles per workgroup
    if V == 4097:
        assert ntok % 32 != 0
    feat = _bf16(torch.randn(B, E, generator=torch.Generator().manual_seed(seed)))
    # oracle, float64
    po = {k: v.double().requires_grad_(True) for k, v in params.items()}
    fo = feat.double().requires_grad_(True)
    lo, _, _ = R.gru_train_loss(po, fo, cap, lens, cell)
    lo.backward()
    for fused in ("1", "0"):
        monkeypatch.setenv("ST_FUSED_CE", fused)
        m = _decoder(cell, params, torch.bfloat16, E, H, V, L).train()
        fd = feat.cuda().requires_grad_(True)
        loss = m.loss(fd, cap.cuda(), lens)
        loss.backward()
        torch.cuda.synchronize()
        tag = f"A {cell} V={V} B={B} L={L} fused={fused}"
        lerr = abs(loss.item() - lo.item()) / abs(lo.item())
        print(f"MEASURE {tag} loss: rel {lerr:.2e}")
        assert lerr < LOSS_REL
        for k, p in m.named_parameters():
            _check_grads(p.grad, po[k].grad, f"{tag} {k}")
        # d loss / d feat per sample: a row depends on its own tokens only, so a stale or missing token tile moves rows
        rerr = _row_l2(fd.grad, fo.grad)
        print(f"MEASURE {tag} dfeat rows: worst rel_l2 {rerr:.2e}")
        assert rerr < ROW_L2
        # d loss / d linear.bias = per-entry column sums of softmax - onehot: a missing 128-entry tile moves its entries ~1/V
        gb, rb = m.linear.bias.grad.double().cpu(), po["linear.bias"].grad
        berr = ((gb - rb).abs().max() / rb.abs().max()).item()
        print(f"MEASURE {tag} linear.bias elementwise: {berr:.2e} of max|ref|")
        assert berr < BIAS_ELEM


# ====================================================================================================================
# B. one bf16 configs[1] training step: head (split-K) -> decoder -> fused CE -> backward -> SGD(momentum)
# ====================================================================================================================

@pytest.mark.parametrize("cell", ["gru", "lstm"])
@pytest.mark.parametrize("B", [128, 100])
def test_configs1_bf16_training_step_matches_fp64_oracle(cell, B, monkeypatch):
    from showtell_amd import optim
    from showtell_amd.head import linear_bn1d
    monkeypatch.setenv("ST_FUSED_CE", "1")
    Fd, L, V, lr, mom, bn_m = 2048, 5, 10000, 0.5, 0.9, 0.01
    g = torch.Generator().manual_seed(40 + B)
    x = _bf16(torch.randn(B, Fd, generator=g).abs())        # post-ReLU average-pool-like features
    w = _bf16(torch.randn(E, Fd, generator=g) * 0.05)       # cnn.py:41
    b = (torch.rand(E, generator=g) * 2 - 1) / math.sqrt(Fd)
    gam = torch.rand(E, generator=g) + 0.5
    bet = torch.randn(E, generator=g) * 0.1
    rm0 = torch.randn(E, generator=g) * 0.1
    rv0 = torch.rand(E, generator=g) + 0.5
    dec = _bf16_params(R.init_decoder_params(E, H, V, L, cell, seed=40 + B))
    if B == 128:
        cap, lens = R.synthetic_captions(B, V, seed=40)
    else:
        cap, lens = _captions(_ragged_lens_100(), V, seed=41)

    # ---- HIP: modules, not the Trainer
    lin, bn = nn.Linear(Fd, E), nn.BatchNorm1d(E, momentum=bn_m)
    with torch.no_grad():
        lin.weight.copy_(w); lin.bias.copy_(b); bn.weight.copy_(gam); bn.bias.copy_(bet)
        bn.running_mean.copy_(rm0); bn.running_var.copy_(rv0)
    lin, bn = lin.cuda(), bn.cuda()
    rnn = _decoder(cell, dec, torch.bfloat16, E, H, V, L).train()
    head_params = [("linear_secondlast_layer.weight", lin.weight), ("linear_secondlast_layer.bias", lin.bias),
                   ("last_layer.weight", bn.weight), ("last_layer.bias", bn.bias)]
    named = head_params + list(rnn.named_parameters())
    opt = optim.SGD([p for _, p in named], lr=lr, momentum=mom)
    opt.zero_grad()
    before = {k: p.detach().double().cpu().clone() for k, p in named}
    y = linear_bn1d(x.cuda(), lin, bn, True, torch.bfloat16)      # F = 2048, E = 512 in bf16: the split-K route
    y.retain_grad()
    loss = rnn.loss(y, cap.cuda(), lens)
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().double().cpu().clone() for k, p in named}
    dy = y.grad.detach().double().cpu()
    opt.step()
    torch.cuda.synchronize()
    after = {k: p.detach().double().cpu() for k, p in named}

    # ---- oracle, float64: encoder head (cnn.py:48-49) -> main.py:145-149 -> torch.optim.SGD
    po = {"linear_secondlast_layer.weight": w.double(), "linear_secondlast_layer.bias": b.double(),
          "last_layer.weight": gam.double(), "last_layer.bias": bet.double()}
    po.update({k: v.double() for k, v in dec.items()})
    po = {k: v.clone().requires_grad_(True) for k, v in po.items()}
    rm, rv = rm0.double().clone(), rv0.double().clone()
    z = x.double() @ po["linear_secondlast_layer.weight"].t() + po["linear_secondlast_layer.bias"]
    z.retain_grad()
    yo = F.batch_norm(z, rm, rv, po["last_layer.weight"], po["last_layer.bias"], True, bn_m, 1e-5)
    yo.retain_grad()
    lo, _, _ = R.gru_train_loss({k: v for k, v in po.items() if not k.startswith(("linear_second", "last_"))}, yo, cap, lens, cell)
    lo.backward()

    tag = f"B {cell} B={B}"
    lerr = abs(loss.item() - lo.item()) / abs(lo.item())
    print(f"MEASURE {tag} loss: rel {lerr:.2e}")
    assert lerr < LOSS_REL
    # the gradient into the head, per sample (the decoder's feature gradient)
    rerr = _row_l2(dy, yo.grad)
    print(f"MEASURE {tag} dy rows: worst rel_l2 {rerr:.2e}")
    assert rerr < ROW_L2
    # Linear bias under batch-statistics BN: the gradient is analytically zero (the oracle's value is float64 noise);
    # bound it by the per-entry sum of |dL/dz| it cancels, and its update likewise
    scale = z.grad.abs().sum(0).max().item()
    kb = "linear_secondlast_layer.bias"
    berr = grads[kb].abs().max().item() / scale
    uerr = (after[kb] - before[kb]).abs().max().item() / (lr * scale)
    print(f"MEASURE {tag} {kb}: |grad| {berr:.2e}, |update| {uerr:.2e} of the cancelled sum")
    assert berr < BIAS_ELEM and uerr < BIAS_ELEM
    for k, p in po.items():
        if k == kb:
            continue
        _check_grads(grads[k], p.grad, f"{tag} grad {k}")
        # the SGD step: torch.optim.SGD's first step with momentum (buffer = gradient)
        with torch.no_grad():
            ref = p.detach().clone()
            R.sgd_momentum_step(ref, p.grad, None, lr, mom)
        _check_update(after[k], before[k], ref, f"{tag} update {k}")
    # BN1d running statistics (momentum 0.01, unbiased variance): the batch statistic each absorbed
    for name, run, r0, ref in (("running_mean", bn.running_mean, rm0, rm), ("running_var", bn.running_var, rv0, rv)):
        got = (run.double().cpu() - (1 - bn_m) * r0.double()) / bn_m
        want = (ref - (1 - bn_m) * r0.double()) / bn_m
        _check_grads(got, want, f"{tag} batch statistic of {name}")
    assert int(bn.num_batches_tracked) == 1


# ====================================================================================================================
# C. greedy decoding (pipe and launch chain) against the bf16-storage oracle
# ====================================================================================================================

def _route():
    from showtell_amd._lib import lib
    return lib().st_rnn_greedy_last_route()


def assert_pipe_ran():
    """after an ST_DECODE_PIPE=1 decode that is eligible for the pipe: route 0.  Route 2 (the pipe gave up: no co-resident
    grid or uneven XCD placement) depends on the machine -- skip, so that the record shows the pipe was not tested."""
    r = _route()
    if r == 2:
        pytest.skip("the pipelined decoder gave up on this machine (route 2): the pipe was NOT tested")
    assert r == 0, f"st_rnn_greedy_last_route() = {r}: the pipelined decoder did not run"


def _greedy_params(cell, V, L, seed):
    """the existing pipe test's weight scaling (a default-initialised stack decodes to a few constant tokens), bf16-rounded"""
    sd = R.init_decoder_params(E, H, V, L, cell, seed=seed)
    sd["linear.weight"] *= 6.0
    if cell == "lstm":
        for k in sd:
            if k.startswith("unit.weight"):
                sd[k] = sd[k] * 5.0
    return _bf16_params(sd)


DELTA = 2.0 ** -7          # divergence tolerance, relative to max |logit| of the step; measured worst 2.1e-3
AGREE = 0.9                # fraction of rows that must agree over all 25 steps; measured lowest 31/33 (0.94)


def _greedy_bounds(cell, L):
    """(DELTA, AGREE) for a decoder.  The 5-layer LSTM with the pipe test's x5 recurrent weights is sensitive: a bf16
    rounding of h or c that an fp32 sum decides differently from the float64 one grows over the steps.  The SAME
    restatement computed in fp32 instead of float64 (same bf16 storage) agrees with the float64 oracle on only 98/128,
    197/256 and 24/33 rows of these cases, with gaps at a divergence up to 1.1e-2 of max|logit|: that is the floor of
    any fp32 implementation.  The kernels (pipe and chain alike) measured at worst 98/128 rows (0.77) and a gap of 2.0e-2
    (B = 256, V = 12288, step 23); these cases get 2^-5 and 2/3."""
    if cell == "lstm" and L == 5:
        return 2.0 ** -5, 2.0 / 3.0
    return DELTA, AGREE


def _check_against_storage_oracle(ids, ids_o, lg_o, tag, delta=DELTA, agree_min=AGREE):
    """Rows agree up to their first differing step; there the kernel's token must be within DELTA * max|logit| of the
    oracle's top logit (a near tie decided by rounding); the row is not compared after that step."""
    B = ids.shape[0]
    agree, worst = 0, 0.0
    for b in range(B):
        d = (ids[b] != ids_o[b]).nonzero()
        if len(d) == 0:
            agree += 1
            continue
        s = int(d[0])
        lg = lg_o[b, s]
        gap = (lg.max() - lg[ids[b, s]]).item() / lg.abs().max().item()
        worst = max(worst, gap)
        assert gap <= delta, (tag, b, s, gap)
    print(f"MEASURE {tag}: {agree}/{B} rows agree over all steps, worst gap at a divergence {worst:.2e} of max|logit|")
    assert agree >= agree_min * B, (tag, agree, B)


@pytest.mark.parametrize("cell", ["gru", "lstm"])
@pytest.mark.parametrize("L,V", [(5, 10000), (5, 12288), (1, 12000)])
@pytest.mark.parametrize("B", [128, 256, 33, 1])
def test_greedy_decoder_matches_bf16_storage_oracle(B, L, V, cell, monkeypatch):
    """(5, 12288) is the pipe's last eligible vocabulary at L = 5 (8 16-entry tiles per vocabulary workgroup)."""
    sd = _greedy_params(cell, V, L, seed=60 + B + L)
    feat = _bf16(torch.randn(B, E, generator=torch.Generator().manual_seed(61 + B)))
    with torch.no_grad():
        ids_o, lg_o = R.rnn_greedy_bf16_storage({k: v.double() for k, v in sd.items()}, feat.double(), cell)
    m = _decoder(cell, sd, torch.bfloat16, E, H, V, L).eval()
    for pipe in ("0", "1"):
        monkeypatch.setenv("ST_DECODE_PIPE", pipe)
        ids = m.sentence_index(feat.cuda()).reshape(B, -1).cpu()
        if pipe == "1":
            assert_pipe_ran()
        else:
            assert _route() == 1
        assert ids.shape == (B, 25)
        _check_against_storage_oracle(ids, ids_o, lg_o, f"C {cell} B={B} L={L} V={V} pipe={pipe}", *_greedy_bounds(cell, L))


# ====================================================================================================================
# D. arg-max ties: the first maximal index on every route
# ====================================================================================================================

def _tie_sets(V):
    return {"pair": [5, V - 3],
            # 9: same 16-entry tile as 5, another lane quad (the shuffle merge); 21: next 16-entry tile (another wave);
            # 70: next 64-entry slice; 133: next 128-entry tile; then the middle and the end of the vocabulary
            "many": [5, 9, 21, 70, 133, V // 2 + 1, V - 3]}


def _with_ties(sd, ties, beta):
    sd = {k: v.clone() for k, v in sd.items()}
    sd["linear.weight"][ties] = 0.0           # logits of the tie entries are exactly the bias on every route
    sd["linear.bias"][ties] = beta
    return sd


def _pick_beta(run, sd, ties):
    """beta from an oracle run with the tie entries out of the race: the median of the other entries' top logit per
    (row, step); then check on the oracle that the tie wins at some steps but not all"""
    lg = run(_with_ties(sd, ties, -1e4))[1]
    beta = float(torch.quantile(lg.max(-1)[0].double().flatten(), 0.5).float())     # the bias is fp32 on every route
    ids = run(_with_ties(sd, ties, beta))[0]
    frac = (ids == ties[0]).double().mean().item()
    assert 0.02 < frac < 0.9, ("tie set-up: the tie must win at some steps but not all", frac)
    return beta


def _assert_tie_rule(ids, ties):
    ids = ids.reshape(-1)
    for k in ties[1:]:
        assert not (ids == k).any(), f"entry {k} tied with {ties[0]} and won: not the first maximal index"
    assert (ids == ties[0]).any(), "the tie never won: the test did not exercise it"


@pytest.mark.parametrize("ties_kind", ["pair", "many"])
@pytest.mark.parametrize("route", ["bf16_pipe", "bf16_chain", "f32_h256_lds", "f32_h512_plain", "logits", "attention"])
def test_argmax_ties_resolve_to_first_index(route, ties_kind, monkeypatch):
    cell, L, V = "gru", 2, 10000
    ties = _tie_sets(V)[ties_kind]
    if route == "attention":
        Ea, Fd, A, Ha, Va, P, B = 128, 256, 128, 128, 3000, 49, 8
        ties = _tie_sets(Va)[ties_kind]
        sd = R.init_decoder_params(Ea, Ha, Va, L, cell, seed=71, attn=dict(F=Fd, A=A))
        sd["linear.weight"] *= 6.0
        feat = torch.randn(B, Fd, P, generator=torch.Generator().manual_seed(71)).abs()

        def run(p):
            with torch.no_grad():
                ids = R.attn_greedy(p, feat, start_id=1, cell=cell)
                return ids, _attn_logits(p, feat, ids, cell)
        beta = _pick_beta(run, sd, ties)
        sd = _with_ties(sd, ties, beta)
        from showtell_amd.rnn_attn import RNN_Attn
        m = RNN_Attn(Ea, Fd, A, Ha, Va, L)
        m.load_state_dict(sd)
        m = m.cuda().eval()
        ids = m.sentence_index(feat.cuda(), lambda w: {"<start>": 1}[w]).cpu()
        assert torch.equal(ids, run(sd)[0])
        _assert_tie_rule(ids, ties)
        return
    if route.startswith("bf16"):
        Hd, dtype, B = 512, torch.bfloat16, 64
        sd = _greedy_params(cell, V, L, seed=72)
        feat = _bf16(torch.randn(B, Hd, generator=torch.Generator().manual_seed(72)))

        def run(p):
            with torch.no_grad():
                return R.rnn_greedy_bf16_storage({k: v.double() for k, v in p.items()}, feat.double(), cell)
    else:
        Hd = 256 if route in ("f32_h256_lds", "logits") else 512     # H > 64 * 4 in fp32: the plain vocab_argmax_kernel
        dtype, B = torch.float32, 32
        sd = R.init_decoder_params(Hd, Hd, V, L, cell, seed=73)
        sd["linear.weight"] *= 6.0
        feat = torch.randn(B, Hd, generator=torch.Generator().manual_seed(73))

        def run(p):
            with torch.no_grad():
                return R.rnn_greedy(p, feat, cell, return_logits=True)
    beta = _pick_beta(run, sd, ties)
    sd = _with_ties(sd, ties, beta)
    m = _decoder(cell, sd, dtype, Hd, Hd, V, L).eval()
    monkeypatch.setenv("ST_DECODE_PIPE", "1" if route == "bf16_pipe" else "0")
    if route == "logits":
        ids, lg = m.sentence_index(feat.cuda(), return_logits=True)
        lg = lg.cpu()
        assert (lg[:, :, ties] == beta).all()                     # zero rows: the logit is the bias, bit for bit
    else:
        ids = m.sentence_index(feat.cuda())
    ids = ids.cpu()
    if route == "bf16_pipe":
        assert_pipe_ran()
    else:
        assert _route() == 1
    if dtype == torch.float32:
        assert torch.equal(ids, run(sd)[0])                       # torch.max: the first maximum
    _assert_tie_rule(ids, ties)


def _attn_logits(params, feat, ids, cell):
    """per-step logits of R.attn_greedy's decode (teacher-forced on its own tokens), for picking beta"""
    B = feat.shape[0]
    h, c = R._attn_init(params, feat, cell)
    fb = feat.transpose(1, 2)
    tok = torch.full((B,), 1, dtype=torch.long)
    out = []
    for t in range(ids.shape[1]):
        z, _ = R.attention_net(params, fb, h[-1])
        ez = z @ params["embed.weight"].t() + params["embed.bias"]
        top, h, c = R.rnn_step(params, torch.cat([params["embeddings.weight"][tok], ez], 1), h, c, cell)
        out.append(top @ params["linear.weight"].t() + params["linear.bias"])
        tok = ids[:, t]
    return torch.stack(out, 1)


# ====================================================================================================================
# E. the greedy route is observable
# ====================================================================================================================

def test_greedy_route_reports_ineligible_calls(monkeypatch):
    from showtell_amd._lib import check, lib
    from showtell_amd.rnn import _cp, _stream
    monkeypatch.setenv("ST_DECODE_PIPE", "1")
    V, L = 1000, 2
    sd = _greedy_params("gru", V, L, seed=80)
    m = _decoder("gru", sd, torch.bfloat16, E, H, V, L).eval()
    feat = _bf16(torch.randn(257, E, generator=torch.Generator().manual_seed(80))).cuda()
    m.sentence_index(feat[:16])                                   # eligible: route 0 (asserted at the end)
    eligible = _route()
    m.sentence_index(feat)                                        # B = 257 > 256
    assert _route() == 1
    m.sentence_index(feat[:16], return_logits=True)               # logits requested
    assert _route() == 1
    prm, keep = m._c_params()                                     # 33 steps: more than the pipe's workspace holds
    nbytes = lib().st_rnn_greedy_workspace_bytes(C.byref(prm), 16)
    ws = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
    ids = torch.empty(16, 33, device="cuda", dtype=torch.long)
    check(lib().st_rnn_greedy(C.byref(prm), _cp(feat[:16]), 16, 33, _cp(ws), nbytes, _cp(ids), None, _stream()), "st_rnn_greedy")
    assert _route() == 1
    m32 = _decoder("gru", R.init_decoder_params(256, 256, V, L, "gru", seed=81), torch.float32, 256, 256, V, L).eval()
    m32.sentence_index(feat[:16, :256].float())                   # fp32, H = 256
    assert _route() == 1
    monkeypatch.setenv("ST_DECODE_PIPE", "0")
    m.sentence_index(feat[:16])
    assert _route() == 1
    if eligible == 2:
        pytest.skip("the pipelined decoder gave up on this machine (route 2): the pipe was NOT tested")
    assert eligible == 0
