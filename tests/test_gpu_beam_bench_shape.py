"""The bf16 beam searches bench.py times, followed record by record by a float64 oracle (oracle/restatement.py on
bf16-representable weights, rounded to bf16 where the kernels store a value).

A free-running comparison cannot be tight: the W-th and (W+1)-th candidate cost of the oracle's own search lie as close
as 3e-8 nats (1 % quantile 3e-4), two correct implementations pick different fringes somewhere.  So the oracle walks the
GPU's OWN records (tok, cost, par, end of every iteration, what beam.replay_hypotheses reads): iteration t is teacher-forced
on tok[t], the oracle's state of slot (b, w) at t + 1 is its own state of slot (b, par[t + 1][b][w]) after that step -- never a value
from the GPU -- and every iteration of every image and slot is checked:

A  bookkeeping, exact: the harvest flags, finished images stay empty, parents are live slots, a live image fills all W
   slots, ascending fringe costs, the root, cost[t + 1] >= cost[t][parent]
B  step cost: cost[t + 1][b][w] - cost[t][b][parent] against the oracle's -log p of that token for that parent (NLL_ABS,
   plus one fp32 spacing of the cumulative cost, which the kernels keep in fp32)
C  selection: over the oracle's candidates cost_gpu[t][b][w'] - log p_oracle(v | w') of all live w' and all v, every chosen
   candidate is within SEL of the oracle's W-th smallest and every candidate more than SEL below it is among the chosen
D  attention maps: the recorded alpha of every live row against the oracle's, row sums, and the alphas handed out with
   each hypothesis are exactly alphas[t - 1][b * W + parent] along its path
E  replay: replay_hypotheses(records) equals beam_search(...) of the same input, for 1 and 3 hypotheses, well formed
F  batch invariance in bf16: images 0..12 of the 256-image search and the 13-image search (both pass A to C) agree on
   the first hypothesis of at least AGREE of the images
G  end to end (BASELINE configs[4]): images -> eval-mode bf16 ResNet-101 + head -> rnn.beam_search.  Covered here: pooled
   features -> head -> search (pooled against the mean of the GPU's own last tap, the head against float64 on the GPU's pooled
   features, the search on the GPU's own features through A to C, the feature tensor reaches beam.py in the encoder's dtype,
   unchanged).  The backbone is not compared here: test_gpu_encoder_bench_shape.py does that block by block.

B and C leave out no live slot (the excluded share is 0 and is asserted).

Inputs.  A default-initialised decoder never emits <end>.  As for bench.py's full-shape beam figure, units of the top layer
are leaky counters that <end> reads (`_counter_unit`); here their update gate also reads the layer below (`gain`) and, in the
attention LSTM, they start at init_c(mean feature), so their pace depends on the image and on the hypothesis.  The input
conditions (share of images that harvest / finish early / never harvest, spread of the first harvest, share of live slots)
are asserted from the float64 oracle's own free-running search, which needs no GPU (`_family`): once per decoder, cell and
beam width, at W = 5 on the first 64 of the 256 images and on the first 13 (plain) / 37 (attention) of them, the small
batches of the cases, and at W = 8 on the case's own 33 / 37 images (inputs of their own).  Every case searches a prefix of
the same 256 images.  B = 1 cannot meet shares by itself (its image is one of the 13); G's 16 features come from a random
encoder and its search's conditions are printed, not asserted.

Runtime.  The whole file takes 52 s on the MI355X machine (16 CPU threads), the float64 oracle included; the floors
(`python -m tests.test_gpu_beam_bench_shape`) take 2.5 minutes on 8 threads.

Bounds.  None comes from the kernels: each is 4x the distance between the SAME bf16-storage restatement evaluated in fp32
and in float64 arithmetic, teacher-forced on the float64 oracle's free-running records of all 256 images
(`python -m tests.test_gpu_beam_bench_shape` prints them; the floor of any implementation that accumulates in fp32).
The kernels' worst measured values on the MI355X follow each constant after the "#".

Mutation checks (each fault injected once into a scratch build of the library and run over the plain GRU cases B = 250, 253
and 13 and F; not committed; measured before the image set was rotated by one place).  NLL_ABS of
these cases is 0.061 (words) / 0.30 (all tokens) nats, SEL 0.60:
  * beam_select_kernel: gather[...] one slot off for w = W - 1 (the child inherits slot W - 2's state)
      B fails at all three sizes: 2.1 nats on words, 9.0 on <end> (B = 13: 1.6 / 2.7); C fails: a chosen candidate 7.8 nats
      above the oracle's W-th, a candidate 3.7 nats below it missed.  A, E, F pass (13/13: the search stays self-consistent).
  * beam_select_kernel: k - 1 - j -> j in the token look-up (the cost keeps its own entry)
      B fails from iteration 0 on: 5.3 nats (B = 13: 4.6); C fails: 5.2 above / 5.1 below.  A, E, F pass.
  * beam_select_kernel: -log taken of top_p of the next slot's row
      B fails from iteration 0 on: 5.2 nats (B = 13: 4.3); C fails: 2.3 above / 3.6 below.  A, E, F pass.
  * rnn_gemm_kernel<.., MT = 2>: a row tile that is not wholly inside M is not written (the last partial tile skipped)
      B = 253 (one row in the second tile of the last workgroup): B fails by 9.4 nats in image 252, C by 10.5 / 2.2.
      B = 250 (two rows in the first tile): E fails first -- two searches of the same input differ in image 249, whose state
      rows are never written.  B = 13 (MT = 1) passes, as it must.
F alone is moved by none of the four (a fault that is the same in both batch sizes keeps them equal); it is there for a
fault that depends on the tiling, and A to C of the two searches carry the weight.
The LSTM and attention bounds are wider (their floors are: words 1.1, all tokens 1.5, SEL 3.1 nats for the plain LSTM; 0.99 /
1.6 / 3.2 attention LSTM; 2.3 / 2.4 / 4.8 attention LSTM at W = 8; 0.16 / 0.48 / 0.97 attention GRU), so the gather and the
wrong-row fault were also run against plain LSTM B = 250, attention GRU and LSTM B = 37 (W = 5), attention LSTM W = 8 and the
plain GRU V = 10003, W = 8 case.  Every case fails under both faults:
  * gather one slot off: B words / all tokens, C above / below the W-th, in nats -- plain LSTM 9.6 / 52.5, 48.2 / 9.8;
    attention GRU 3.0 / 3.0, 2.4 / 0.28 (alpha off by 1.9e-4, 5x its bound); attention LSTM 12.2 / 12.2, 7.7 / 2.8 (alpha
    2.3e-3, 8x); attention LSTM W = 8 11.8 / 29.7, 27.9 / 4.7; plain GRU W = 8 0.91 / 3.7, 3.0 / 1.2
  * -log of the next slot's row: plain LSTM 6.8 / 6.8, 7.8 / 6.4; attention GRU 1.8 / 1.8, 0.54 / 1.3; attention LSTM 8.3 / 8.3,
    5.0 / 2.0; attention LSTM W = 8 7.4 / 7.4, 4.9 / 6.1 (alpha unmoved, as it must be); plain GRU W = 8 4.2 / 5.2, 2.4 / 1.9
"""
import numpy as np
import pytest
import torch

from oracle import restatement as R
from tests._beam_oracle import StepOracle, beam_distance, check_records
from tests.test_gpu_attention_beam import _config3, _make
from tests.test_gpu_decoder_bench_shape import _bf16, _bf16_params, _decoder

pytestmark = pytest.mark.gpu

E = H = 512
L, V, T = 5, 10000, 25
START, END = 1, 2
# the input conditions are asserted on the first n images for every n listed: 64 and the small batch of the W = 5 cases (F's 13
# plain images, the 37 attention images), the case's own batch at W = 8
COND_IMAGES = {("plain", 5): (64, 13), ("attn", 5): (64, 37), ("plain", 8): (33,), ("attn", 8): (37,)}
# the 256 random images are rotated by this many places, so that these prefixes meet the conditions (searched on the CPU)
ROTATE = {"plain": 255, "attn": 242}

# The counter unit of each decoder family: vocabulary scale, recurrent scale, <end>'s weight on the counter, <end> bias boost,
# gain of the update gate on the layer below, spread of the counter's start over the images.  Chosen on the CPU so that the
# oracle alone meets the input conditions.
COUNTER = {
    ("plain", "gru", 5): dict(lin=12.0, rec=1.25, endw=21.0, boost=-12.5, gain=0.7),
    ("plain", "lstm", 5): dict(lin=6.0, rec=5.0, endw=200.0, boost=-136.0, gain=0.25),
    ("attn", "gru", 5): dict(lin=1.0, rec=1.0, endw=100.0, boost=-64.0, gain=0.5),        # _config3 has scaled the vocabulary x12
    ("attn", "lstm", 5): dict(lin=0.5, rec=5.0, endw=160.0, boost=-94.0, gain=0.05, start=2.0),
    # W = 8 (V = 10003, 33 images; attention, 37 images): an image is finished only when all 8 slots end in the same iteration
    # plain: little separates the images at W = 8, so <end> also reads a latch of the feature step (`latch`, see _counter_unit)
    ("plain", "gru", 8): dict(lin=12.0, rec=1.0, endw=60.0, boost=-42.0, gain=0.3, latch=8.0, latch_gain=8.0),
    ("attn", "gru", 8): dict(lin=1.0, rec=1.0, endw=100.0, boost=-64.0, gain=0.5),
    ("attn", "lstm", 8): dict(lin=0.5, rec=5.0, endw=240.0, boost=-140.0, gain=0.05, start=2.0),
}

# B: (tokens other than <end>, every token): 4 x the floor in nats, fp32 against float64 arithmetic of the storage oracle on its
# own 256-image records (`python -m tests.test_gpu_beam_bench_shape`).  <end> has a floor of its own: its logit reads the
# counters, whose pace integrates the layer below over the steps, so storage roundings that fp32 and float64 sums decide
# differently add up coherently in it.  The 5-layer LSTMs
# with x5 recurrent weights amplify such a rounding over the steps (as _greedy_bounds of the decoder file found for greedy).
NLL_ABS = {
    ("plain", "gru", 5): (4 * 1.52e-2, 4 * 7.55e-2),      # 1.14e-2, 7.06e-2 (B = 256; configs[4] end to end: 7.6e-3, 3.2e-2)
    ("plain", "lstm", 5): (4 * 2.81e-1, 4 * 3.87e-1),     # 1.64e-1, 2.71e-1 (B = 256)
    ("attn", "gru", 5): (4 * 4.04e-2, 4 * 1.21e-1),       # 6.45e-2, 2.02e-1 (B = 256)
    ("attn", "lstm", 5): (4 * 2.47e-1, 4 * 3.99e-1),      # 2.44e-1, 2.98e-1 (B = 256)
    # W = 8: inputs of their own (COUNTER), floors on the case's own 33 / 37 images
    ("plain", "gru", 8): (4 * 1.91e-2, 4 * 3.72e-2),      # 2.42e-2, 2.42e-2
    ("attn", "gru", 8): (4 * 2.70e-2, 4 * 1.14e-1),       # 2.72e-2, 1.11e-1
    ("attn", "lstm", 8): (4 * 5.74e-1, 4 * 5.94e-1),      # 3.38e-1, 6.31e-1
}
NLL_ABS_F32 = (4 * 7.7e-6, 4 * 4.72e-5)                   # fp32 kernels, unrounded float64 oracle: 3.2e-6, 4.32e-5
# D: 4 x the floors of the attention families: (max |d alpha|, worst per-row relative L2)
ALPHA = {
    ("gru", 5): (4 * 9.6e-6, 4 * 1.54e-4),                # 1.04e-5, 1.43e-4
    ("lstm", 5): (4 * 7.5e-5, 4 * 1.24e-3),               # 8.1e-5, 1.22e-3
    ("gru", 8): (4 * 7.6e-6, 4 * 1.08e-4),                # 8.8e-6, 1.14e-4
    ("lstm", 8): (4 * 5.4e-5, 4 * 9.0e-4),                # 5.3e-5, 1.00e-3
}
# F: share of the 256 images whose first hypothesis the float64 and the fp32-arithmetic free-running oracle share (0.980, 0.957),
# minus 0.1
AGREE = {"gru": 0.980 - 0.1, "lstm": 0.957 - 0.1}       # 13/13, 13/13

_CACHE = {}


# ====================================================================================================================
# inputs
# ====================================================================================================================

NCOUNT = 128      # counter units; <end> reads each with endw / NCOUNT: ONE bf16 step of one of them (2^-8) moves its logit little


NLATCH = 16


def _counter_unit(sd, cell, lin, rec, endw, boost, gain, start=0.0, latch=0.0, latch_gain=0.25):
    """Units 0..NCOUNT-1 of the top layer become leaky counters (each keeps ~0.9 of itself and moves towards tanh(3)) that
    listen to nothing but, through their update gate, the layer below (ONE fixed random row x gain, so they keep pace;
    gate biases spread by +-0.1, so their values differ); <end> reads their mean with weight endw and gets `boost` on its
    bias, no other token reads them; every other weight stays random.  bf16-rounded.

    One counter read with the whole weight (bench.py's construction) makes -log p(<end>) hang on a single stored value: its
    bf16 step 2^-8 x endw is 0.08 nats at endw = 21 and 0.6 at 160, and that was the whole fp32-against-float64 floor of the
    oracle (measured: 0.083 and 0.63 nats, one flipped rounding of the counter somewhere in 32000 slots)."""
    Ln = R.num_layers_of(sd)
    Hd = sd["unit.weight_hh_l0"].shape[1]
    top = "_l%d" % (Ln - 1)
    G = 3 if cell == "gru" else 4
    K = NCOUNT
    sd = {k: v.clone() for k, v in sd.items()}
    sd["linear.weight"] = sd["linear.weight"] * lin
    for k in sd:
        if k.startswith("unit.weight"):
            sd[k] = sd[k] * rec
    wi, wh, bi, bh = (sd[n + top] for n in ("unit.weight_ih", "unit.weight_hh", "unit.bias_ih", "unit.bias_hh"))
    row = torch.randn(wi.shape[1], generator=torch.Generator().manual_seed(5)) * gain
    keep = 2.1972 + torch.linspace(-0.1, 0.1, K)
    for gate in range(G):
        wi[gate * Hd:gate * Hd + K] = 0.0; wh[gate * Hd:gate * Hd + K] = 0.0
        bi[gate * Hd:gate * Hd + K] = 0.0; bh[gate * Hd:gate * Hd + K] = 0.0
    if cell == "gru":                                   # gates r, z, n: h' = (1 - z) n + z h
        bi[Hd:Hd + K] = keep; wi[Hd:Hd + K] = row
        bi[2 * Hd:2 * Hd + K] = 3.0
    else:                                               # gates i, f, g, o: c' = f c + i g, h = o tanh(c)
        bi[0:K] = -keep; wi[0:K] = -row
        bi[Hd:Hd + K] = keep; wi[Hd:Hd + K] = row
        bi[2 * Hd:2 * Hd + K] = 3.0
        bi[3 * Hd:3 * Hd + K] = 6.0
    if start:                                   # attention: the counters start at init(mean feature), N(0, ~start^2) per image
        k = "init_h" if cell == "gru" else "init_c"
        r0 = torch.randn(sd[k + ".weight"].shape[1], generator=torch.Generator().manual_seed(6))
        sd[k + ".weight"][:K] = (r0 - r0.mean()) * (start / (0.0861 * r0.numel() ** 0.5))   # the mean of 49 |N(0, 1)|: std 0.0861
        sd[k + ".bias"][:K] = 0.0
    sd["linear.weight"][:, :K] = 0.0
    sd["linear.weight"][END, :K] = endw / K
    sd["linear.bias"][END] += boost
    if latch:
        # plain GRU: units K..K+NLATCH-1 of the top layer latch the image.  Their update gate reads the counters only:
        # z = sigmoid(-4 + 80 mean(counters)), open at the feature step (all counters 0) and shut from the next step on, so they
        # keep n = tanh(latch_gain x row . layer below) of the feature step: one value per image, the same in all its slots.
        # <end> reads their mean with weight `latch`: an image-dependent <end> bias.
        assert cell == "gru"
        J = slice(K, K + NLATCH)
        lrow = torch.randn(wi.shape[1], generator=torch.Generator().manual_seed(7)) * latch_gain
        for gate in range(3):
            wi[gate * Hd + K:gate * Hd + K + NLATCH] = 0.0; wh[gate * Hd + K:gate * Hd + K + NLATCH] = 0.0
            bi[gate * Hd + K:gate * Hd + K + NLATCH] = 0.0; bh[gate * Hd + K:gate * Hd + K + NLATCH] = 0.0
        bi[Hd + K:Hd + K + NLATCH] = -4.0
        wh[Hd + K:Hd + K + NLATCH, :K] = 80.0 / K
        wi[2 * Hd + K:2 * Hd + K + NLATCH] = lrow[None, :] * torch.linspace(0.8, 1.2, NLATCH)[:, None]
        sd["linear.weight"][:, J] = 0.0
        sd["linear.weight"][END, J] = latch / NLATCH
    return _bf16_params(sd)


def _conditions(rec):
    """the input conditions of a search, from its records"""
    end, cost = rec["end"].astype(bool), rec["cost"]
    Tn, B, W = end.shape
    done, nlive = np.zeros(B, bool), 0
    for t in range(Tn):
        live = np.isfinite(cost[t]) & ~end[t] & ~done[:, None]
        done = done | ~live.any(1)
        nlive += int((live & ~done[:, None]).sum())
    first = [int(np.nonzero(end[:, b].any(1))[0][0]) if end[:, b].any() else -1 for b in range(B)]
    return dict(harvest=float(np.mean([f >= 0 for f in first])), done=float(done.mean()),
                never=sum(1 for f in first if f < 0 or f == Tn - 1), distinct=len({f for f in first if f >= 0}),
                live=nlive / float(Tn * B * W))


def _assert_conditions(c, tag):
    print(f"MEASURE {tag} input conditions on the oracle alone: {c}")
    assert c["harvest"] >= 0.75, (tag, c)           # at least 3/4 of the images harvest a hypothesis
    assert c["done"] >= 0.125, (tag, c)             # at least 1/8 are finished before iteration T
    assert c["never"] >= 1, (tag, c)                # one never harvests, or only at the last checkable iteration
    assert c["distinct"] >= 5, (tag, c)             # first-harvest iterations span at least 5 values
    assert c["live"] >= 0.4, (tag, c)               # at least 40 % of all (iteration, image, slot) entries are live


def _base_params(kind, cell, Vv):
    if kind == "plain":
        return R.init_decoder_params(E, H, Vv, L, cell, seed=5)
    assert Vv == V
    return _config3(cell, 1)[0]


def _family(kind, cell, Vv=V, W=5, conditions=True):
    """(params, feat of 256 images), both fp32 and bf16-representable; the input conditions are asserted once per family
    (decoder, cell, beam width) from the float64 oracle's free-running search of every prefix COND_IMAGES lists"""
    key = (kind, cell, Vv, W)
    if key not in _CACHE:
        params = _counter_unit(_base_params(kind, cell, Vv), cell, **COUNTER[(kind, cell, W)])
        g = torch.Generator().manual_seed(5)
        feat = _bf16(torch.randn(256, E, generator=g) if kind == "plain" else torch.randn(256, 2048, 49, generator=g).abs())
        _CACHE[key] = [params, torch.roll(feat, -ROTATE[kind], 0), None]
    ent = _CACHE[key]
    if conditions and ent[2] is None:
        ent[2] = [_conditions(StepOracle(kind, cell, ent[0], ent[1][:n], W, True).free_run(T)) for n in COND_IMAGES[(kind, W)]]
        for n, c in zip(COND_IMAGES[(kind, W)], ent[2]):
            _assert_conditions(c, f"{kind} {cell} V={Vv} W={W} first {n} images")
    return ent[0], ent[1]


# ====================================================================================================================
# the checker (A to D on one search's records: tests/_beam_oracle.check_records), hypotheses, paths
# ====================================================================================================================

def _check_hypotheses(hyps, nh):
    for hyp in hyps:
        assert len(hyp) <= nh
        costs = [h[1] for h in hyp]
        assert costs == sorted(costs)
        for h in hyp:
            assert h[0][0] == START and h[0][-1] == END and len(h[0]) <= T + 1 and np.isfinite(h[1])


def _paths(rec, b):
    """every harvested node of image b: ((tokens), cost) -> [(t, slot)] from the first node after the root to the node itself"""
    out = {}
    for t, w in zip(*np.nonzero(rec["end"][:, b])):
        c, seq, path = float(rec["cost"][t, b, w]), [], []
        while t >= 0:
            seq.append(int(rec["tok"][t, b, w]))
            if t > 0:
                path.append((int(t), int(w)))
                w = rec["par"][t, b, w]
            t -= 1
        out.setdefault((tuple(seq[::-1]), c), path[::-1])
    return out


# ====================================================================================================================
# searches on the GPU
# ====================================================================================================================

def _plain_model(cell, params, dtype, Vv=V):
    key = ("model", cell, dtype, Vv)
    if key not in _CACHE:
        _CACHE[key] = _decoder(cell, params, dtype, E, H, Vv, L).eval()
    return _CACHE[key]


def _plain_search(cell, B, W=5, Vv=V, dtype=torch.bfloat16):
    """records of the plain decoder's search on the first B images (cached: F reads the B = 256 and B = 13 ones again) and
    check E"""
    from showtell_amd.beam import beam_search, beam_search_records, replay_hypotheses
    key = ("rec", cell, B, W, Vv, dtype)
    if key not in _CACHE:
        params, feat = _family("plain", cell, Vv, W)
        m = _plain_model(cell, params, dtype, Vv)
        f = feat[:B].cuda()                                   # fp32 in: beam.py casts it to the compute dtype
        rec = beam_search_records(m, f, W, T, START, END)
        for nh in (1, 3):                                     # E
            hyps = m.beam_search(f, W, nh, T, START, END)
            assert hyps == replay_hypotheses(rec["tok"], rec["cost"], rec["par"], rec["end"], nh) == beam_search(m, f, W, nh, T)
            _check_hypotheses(hyps, nh)
        _CACHE[key] = rec
    return _CACHE[key]


# rows of a step = B * W.  rnn_gemm_launch_batch takes rnn_gemm_kernel<.., MT = 2> (32 rows per workgroup, two 16-row tiles)
# for a single cell from 512 rows on, MT = 1 (16 rows) below
PLAIN_CASES = [("gru", 256), ("gru", 250), ("gru", 253), ("gru", 103), ("gru", 102), ("gru", 13), ("gru", 1),
               ("lstm", 256), ("lstm", 250), ("lstm", 253), ("lstm", 13), ("lstm", 1)]


@pytest.mark.parametrize("cell,B", PLAIN_CASES)
def test_plain_beam5_records_follow_the_storage_oracle(cell, B):
    rows = B * 5
    assert {256: rows == 40 * 32, 250: rows == 39 * 32 + 2, 253: rows == 39 * 32 + 17, 103: 512 <= rows < 512 + 16,
            102: 512 - 16 < rows < 512, 13: rows < 512, 1: rows < 16}[B]
    params, feat = _family("plain", cell)
    rec = _plain_search(cell, B)
    check_records(rec, StepOracle("plain", cell, params, feat[:B], 5, True), NLL_ABS[("plain", cell, 5)], f"plain {cell} B={B} W=5")


def test_plain_gru_ragged_vocabulary_width8():
    """V = 10003 (Vp = 10008: a ragged last vocabulary tile), W = 8: softmax_topk's k = 8 route and W * k = 64, the limit of
    st_beam_select; 33 images."""
    Vv, W, B = 10003, 8, 33
    assert COND_IMAGES[("plain", W)] == (B,)              # the input conditions are asserted on these 33 images
    params, feat = _family("plain", "gru", Vv, W)
    rec = _plain_search("gru", B, W, Vv)
    check_records(rec, StepOracle("plain", "gru", params, feat[:B], W, True), NLL_ABS[("plain", "gru", W)], "plain gru B=33 W=8 V=10003")


def test_plain_gru_fp32_through_the_same_checker():
    """The fp32 kernels against the unrounded float64 oracle: only the summation order differs.  The floor of the checker."""
    params, feat = _family("plain", "gru")
    rec = _plain_search("gru", 256, dtype=torch.float32)
    check_records(rec, StepOracle("plain", "gru", params, feat, 5, storage=False), NLL_ABS_F32, "plain gru fp32 B=256 W=5")


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_bf16_batch_invariance_of_the_first_hypothesis(cell):
    """F.  The cell tiles 1280 rows differently from 65, so the two searches need not be bit-equal; both pass A to C above."""
    from showtell_amd.beam import replay_hypotheses
    first = []
    for B in (256, 13):
        rec = _plain_search(cell, B)
        hyps = replay_hypotheses(rec["tok"], rec["cost"], rec["par"], rec["end"], 1)
        first.append([h[0][0] if h else None for h in hyps[:13]])
    same = sum(int(a == b) for a, b in zip(*first))
    print(f"MEASURE F plain {cell}: {same}/13 first hypotheses agree between B = 256 and B = 13")
    assert same >= AGREE[cell] * 13


@pytest.mark.parametrize("cell,B,W", [("gru", 256, 5), ("gru", 37, 5), ("gru", 37, 8),
                                      ("lstm", 256, 5), ("lstm", 37, 5), ("lstm", 37, 8)])
def test_attention_beam_records_follow_the_storage_oracle(cell, B, W):
    """config-3 geometry: F = 2048, A = 512, P = 49."""
    from showtell_amd.beam import replay_hypotheses
    params, feat = _family("attn", cell, V, W)
    key = ("model", "attn", cell, W)
    if key not in _CACHE:
        _CACHE[key] = _make(cell, params, torch.bfloat16)
    m = _CACHE[key]
    f = feat[:B].cuda()
    hyps, rec = m.beam_search(f, W, 3, T, START, END, return_alphas=True, return_records=True)
    assert rec["alpha"].shape == (T, B * W, 49) and rec["alpha"].dtype == np.float32
    # E: a second search without records and without maps gives the same hypotheses as the replay of these records
    assert [[(s, c) for s, c, _ in h] for h in hyps] == replay_hypotheses(rec["tok"], rec["cost"], rec["par"], rec["end"], 3)
    assert [[(s, c) for s, c, _ in h] for h in hyps] == m.beam_search(f, W, 3, T, START, END)
    assert [h[:1] for h in m.beam_search(f, W, 3, T, START, END)] == m.beam_search(f, W, 1, T, START, END)
    _check_hypotheses(hyps, 3)
    # D: the maps handed out are exactly alphas[t - 1][b * W + parent slot] along each hypothesis
    for b, hyp in enumerate(hyps):
        paths = _paths(rec, b)
        for s, c, a in hyp:
            want = np.stack([rec["alpha"][t - 1, b * W + rec["par"][t, b, w]] for t, w in paths[(tuple(s), c)]])
            assert a.dtype == torch.float32 and np.array_equal(a.numpy(), want), b
    check_records(rec, StepOracle("attn", cell, params, feat[:B], W, True), NLL_ABS[("attn", cell, W)], f"attention {cell} B={B} W={W}",
                  alpha_bounds=ALPHA[(cell, W)])


# G: the head's output against float64 Linear + BatchNorm1d(eval) of the GPU's pooled features, of max |ref|.  The head's
# input and output are each stored in bf16 (2^-9 relative per value): two roundings, margin 2.  (The encoder file has no
# head bound to reuse; its POOL_MAX holds the pooled features.)
HEAD_MAX = 2.0 ** -7     # 2.15e-3 (pooled: 7.1e-8)


def test_end_to_end_configs4_images_to_beam_search(monkeypatch):
    """G.  16 images -> eval-mode bf16 ResNet(101, 512) and head -> rnn.beam_search.  What this test checks is pooled features
    -> head -> search; the backbone itself is NOT compared here (test_gpu_encoder_bench_shape.py's eval256 does that, block by
    block: a free-running float64 ResNet has no bound, the undamped network amplifies bf16 roundings).  The encoder is followed as
    test_gpu_encoder_bench_shape.py follows it, from the HIP path's own taps: pooled features against the float64 mean of
    the last tap (POOL_MAX of that file), the head against float64 Linear + BatchNorm1d(eval) of the GPU's pooled features.
    The search on the GPU's own features passes A to C; the features reach beam.py in the encoder's dtype, unchanged."""
    from showtell_amd import beam
    from tests.test_gpu_encoder_bench_shape import POOL_MAX, _model, _nchw64, _params
    B = 16
    ep = _params(34)
    image = _bf16(torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(34)))
    cnn = _model(ep, False, False)
    outs, pooled = cnn._bb.block_outputs(image.cuda(), False)
    pref = _nchw64(outs[-1].cpu()).mean((2, 3))
    perr = ((pooled.double().cpu() - pref).abs().max() / pref.abs().max()).item()
    with torch.no_grad():
        y = cnn(image.cuda())
    pd = {k: v.double() for k, v in ep.items() if k.startswith(("linear_secondlast", "last_layer")) and v.is_floating_point()}
    z = pooled.double().cpu() @ pd["linear_secondlast_layer.weight"].t() + pd["linear_secondlast_layer.bias"]
    yref = torch.nn.functional.batch_norm(z, pd["last_layer.running_mean"], pd["last_layer.running_var"], pd["last_layer.weight"],
                                          pd["last_layer.bias"], False, 0.01, 1e-5)
    herr = ((y.double().cpu() - yref).abs().max() / yref.abs().max()).item()
    print(f"MEASURE G pooled {perr:.2e} of max|ref|, head {herr:.2e} of max|ref|, feature dtype {y.dtype}")
    assert perr <= POOL_MAX and herr <= HEAD_MAX
    assert y.dtype in (torch.bfloat16, torch.float32) and y.shape == (B, E)
    params, _ = _family("plain", "gru")
    rnn = _plain_model("gru", params, torch.bfloat16)
    seen = []
    real = beam._feat
    monkeypatch.setattr(beam, "_feat", lambda r, f: (seen.append(f), real(r, f))[1])
    hyps = rnn.beam_search(y, 5, 1, T, START, END)
    rec = beam.beam_search_records(rnn, y, 5, T, START, END)
    assert len(seen) == 2 and all(f is y for f in seen)               # the encoder's tensor itself, no copy or cast before beam.py
    assert hyps == beam.replay_hypotheses(rec["tok"], rec["cost"], rec["par"], rec["end"], 1)
    _check_hypotheses(hyps, 1)
    print("MEASURE G conditions of the GPU's search:", _conditions(rec))
    check_records(rec, StepOracle("plain", "gru", params, y.float().cpu(), 5, True), NLL_ABS[("plain", "gru", 5)], "G configs[4] 16 images")


# ====================================================================================================================
# the floors: `python -m tests.test_gpu_beam_bench_shape [images]` (CPU only)
# ====================================================================================================================

def _floor(kind, cell, B, W=5, Vv=V, storage=True):
    """fp32 against float64 arithmetic of the same restatement, teacher-forced on the float64 oracle's own free-running
    records: max |d nll| over the filled slots, alpha distances over the live rows; and the share of images whose first
    hypothesis the two free-running searches share"""
    from showtell_amd.beam import replay_hypotheses
    params, feat = _family(kind, cell, Vv, W, conditions=False)
    o64 = StepOracle(kind, cell, params, feat[:B], W, storage)
    o32 = StepOracle(kind, cell, params, feat[:B], W, storage, torch.float32)
    gaps = []

    def gap_of(t, out, cost_t, live):
        """distance between the W-th and the (W + 1)-th best candidate cost of every image with live slots"""
        tv = torch.topk(out[0], W + 1, dim=1)[0].double().view(B, W, W + 1).numpy()
        c = np.sort(np.where(live[:, :, None], cost_t[:, :, None] - tv, np.inf).reshape(B, -1), axis=1)
        ok = np.isfinite(c[:, W])
        gaps.append(c[ok, W] - c[ok, W - 1])
    rec = o64.free_run(T, keep=gap_of)
    gap = np.concatenate(gaps)
    out = dict(cond=_conditions(rec), gap_min=float(gap.min()), gap_q01=float(np.quantile(gap, 0.01)), **beam_distance(o32, o64, rec))
    h64 = replay_hypotheses(rec["tok"], rec["cost"], rec["par"], rec["end"], 1)
    r32 = o32.free_run(T)
    h32 = replay_hypotheses(r32["tok"], r32["cost"], r32["par"], r32["end"], 1)
    out["agree"] = float(np.mean([(a[0][0] if a else None) == (b[0][0] if b else None) for a, b in zip(h64, h32)]))
    return out


if __name__ == "__main__":
    import sys
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    for case in [("plain", "gru", n), ("plain", "lstm", n), ("attn", "gru", n), ("attn", "lstm", n),
                 ("plain", "gru", 33, 8, 10003), ("attn", "gru", 37, 8), ("attn", "lstm", 37, 8), ("plain", "gru", n, 5, V, False)]:
        print("FLOOR", case, _floor(*case), flush=True)
