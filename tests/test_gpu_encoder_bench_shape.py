"""The bf16 ResNet-101 encoder bench.py times, against a float64 oracle (oracle/restatement.py on bf16-representable weights).

Configurations (computed once each by the module-scoped fixture, which holds one at a time; the float64 tensors are large):
  b128     B = 128, train: the headline encoder (a train == 2 forward + st_resnet_update_running)
  b127     B = 127, train: every 112-row conv1x1_astat grid at 14 x 14 and 7 x 7 ends in a partial tile, an odd image count;
           the same kernel family on every launch line as B = 128 (asserted from the host-only plan)
  attn64   B = 64, train, cnn_attn.ResNet: the encoder of bench.py's attention configuration
  eval256  B = 256, eval: the encoder of bench.py's beam configuration (8 images checked: per-sample BatchNorm)

Conv weights and images are rounded to bf16 first, BatchNorm parameters and running buffers are random (as
test_gpu_encoder._make(damp=False)), so that what is left between the kernels and the oracle is bf16 storage and summation
order.  The engine hands out every block output as it stored it (st_resnet_set_taps); the oracle computes stem + pool +
block 0 from the image and block k from the HIP path's own tap k - 1 (exact in float64): every comparison sees one block.

A  every block output elementwise: max-rel, L2, and the worst per-image max-rel (a fault in one image, one band or the last
   partial tile is not averaged away)
B  per-channel moments of every block output: |mean_got - mean_ref| / std_ref and |std_got / std_ref - 1|.  Rounding noise
   averages out over 6 k - 401 k samples per channel; a wrong count, eps, gamma / beta or replica sum does not
C  running buffers of all 104 BatchNorm layers: the batch mean and unbiased variance each absorbed, recovered from
   (after - 0.9 before) / 0.1, and num_batches_tracked
D  pooled features against a float64 mean over 7 x 7 of the last tap (fp32 summation, not bf16, error)
E  bench.py's pipelined route (Trainer.step with upcoming = bench.py's ahead()): the closed form of five momentum updates
F  Trainer drops prefetched forwards when the caller changes its mind: their running-buffer updates must not stay

The worst values measured on the MI355X are written next to each bound.
"""
import gc

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import restatement as R
from tests._encoder_walk import KEEP32, MOM32, _absorbed, _batch_stats, _bf16, _block_metrics, _nchw64, _params  # noqa: F401

pytestmark = pytest.mark.gpu

CONFIGS = {
    "b128": dict(B=128, train=True, attn=False, seed=31),
    "b127": dict(B=127, train=True, attn=False, seed=32),
    "attn64": dict(B=64, train=True, attn=True, seed=33),
    "eval256": dict(B=256, train=False, attn=False, seed=34),
}
EVAL_ROWS = [0, 1, 77, 127, 128, 129, 200, 255]      # eval256: the first and last images, those either side of image 128

# A: blocks 1-32 (one block: three bf16 storage roundings + bf16 filters); worst measured over b128 / b127 / attn64, then eval256
BLOCK_MAX = 1.2e-2      # train 6.2e-3 (b127 layer4.0), eval 5.4e-3
BLOCK_L2 = 1e-2         # train 4.7e-3 (b127 layer4.0), eval 2.7e-3
BLOCK_IMG_MAX = 1.6e-2  # train 7.7e-3 (b128 layer3.0), eval 5.5e-3
# block 0 is compared from the IMAGE: the stem's raw output is stored in bf16 before its BatchNorm, then pool and the four
# convolutions of layer1.0 -- about twice the roundings of any other block
BLOCK0_MAX = 2.4e-2     # train 1.1e-2 (b128), eval 5.4e-3
BLOCK0_L2 = 2e-2        # train 1.0e-2 (b128), eval 3.2e-3
BLOCK0_IMG_MAX = 3e-2   # train 1.5e-2 (attn64), eval 5.4e-3
# B: per-channel moments of the block outputs (train configurations)
MOMENT_MEAN = 1e-3      # 5.3e-4 (attn64 layer3.4)
MOMENT_STD = 1.5e-3     # 7.7e-4 (b127 layer3.4)
# C: the batch statistics each running buffer absorbed
RUN_MEAN = 4e-3         # in units of the oracle's std: 1.9e-3 (b127 layer1.0 bn1)
RUN_VAR = 3e-3          # relative: 1.5e-3 (attn64 layer1.0 downsample)
# D: pooled features, relative to max |ref|: fp32 summation of 49 values
POOL_MAX = 2e-7         # 9.0e-8 (attn64)
# E: five pipelined updates against their closed form (recovered statistics as in C).  Unlike C, each of the five forwards is
# a whole forward of its own: its statistics of block k come from its own blocks 0..k-1, whose summation order (fp32 atomics)
# differs from the tapped forward's, and the undamped network amplifies the bf16 rounding flips that follow ~1.25x per block.
# Two plain forwards of the same image, one after the other, differ by as much: 2.2e-2 (mean), 7.0e-2 (variance).  These
# bounds therefore catch only gross errors of the update chain: a lost update shifts the recovered mean by 0.16 (rm0 - mean)
# and the variance by 0.16 (rv0 / var - 1), which is large only where the batch statistics are far from the starting
# buffers (the stem, for one).  Count errors are caught by the exact num_batches_tracked check.
PIPE_MEAN = 4e-2        # 1.9e-2
PIPE_VAR = 1.5e-1       # 7.3e-2
# F: a pipelined run that drops prefetched forwards against the plain loop (whole forwards again: the same amplification)
DROP_MEAN = 1.5e-2      # |d running_mean| / sqrt(running_var): 7.1e-3
DROP_VAR = 1.3e-1       # |d running_var| / running_var: 6.5e-2 (modes)

BNS = [bn for *_, bn in R.resnet_conv_list(101)]


def _model(params, attn, train):
    from showtell_amd.cnn import ResNet
    from showtell_amd.cnn_attn import ResNet as ResNetAttn
    m = (ResNetAttn if attn else ResNet)(101, 512, dtype=torch.bfloat16)
    m.load_state_dict(params)
    return m.cuda().train(train)


def _buffers(m):
    sd = m.state_dict()
    return {k: v.detach().cpu().clone() for k, v in sd.items() if k.startswith("model.") and
            k.endswith(("running_mean", "running_var", "num_batches_tracked"))}


def _run(name):
    """One HIP forward with taps, the float64 oracle block by block, and everything the checks read (small: the taps and the
    oracle's tensors are freed here)."""
    cfg = CONFIGS[name]
    B, train, attn = cfg["B"], cfg["train"], cfg["attn"]
    if name == "b127":
        from tests.test_resnet_plan import fields, plan
        a, b = plan(101, "bf16", 224, 224, 128, True), plan(101, "bf16", 224, 224, 127, True)
        assert len(a) == len(b) and all(fields(x)["family"] == fields(y)["family"] for x, y in zip(a, b)), \
            "B = 127 changes a kernel route: pick another odd B near 128 that keeps them all"
    params = _params(cfg["seed"])
    image = _bf16(torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(cfg["seed"])))
    m = _model(params, attn, train)
    before = _buffers(m)
    res = m._bb.block_outputs(image.cuda(), train, want_ncp=attn)
    outs, pooled = res[0], res[1].cpu()
    after = _buffers(m)
    out = dict(name=name, cfg=cfg, params=params, image=image, before=before, after=after)
    if attn:       # cnn_attn.ResNet's (B, 2048, 49) map of the same forward against the last tap, widened to fp32
        out["ncp_exact"] = torch.equal(res[2], outs[-1].float().permute(0, 3, 1, 2).reshape(B, 2048, 49))
    rows = EVAL_ROWS if not train else list(range(B))
    sel = torch.tensor(rows)
    p = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in params.items()}
    blocks = []
    with torch.no_grad():
        x = image[sel].double()
        xin = F.max_pool2d(F.relu(R._bn2d(p, F.conv2d(x, p["model.0.weight"], None, 2, 3), "model.1", train)), 3, 2, 1)
        k = 0
        for li, nb in enumerate(R.RESNET_SPECS[101][1]):
            for bi in range(nb):
                ref = R.block_forward(p, xin, 101, li, bi, train)
                got = _nchw64(outs[k][sel.to(outs[k].device)].cpu() if not train else outs[k].cpu())
                assert got.shape == ref.shape, (k, got.shape, ref.shape)
                met = _block_metrics(got, ref, moments=train)
                met.update(k=k, name=f"layer{li + 1}.{bi}")
                blocks.append(met)
                del ref, xin
                xin = got
                k += 1
        # D: the pooled features against a float64 mean of the last tap
        pref = xin.mean((2, 3))
        out["pool"] = ((pooled[sel].double() - pref).abs().max() / pref.abs().max()).item()
    out["blocks"] = blocks
    out["oracle"] = {k: v for k, v in p.items() if k.endswith(("running_mean", "running_var", "num_batches_tracked")) and k.startswith("model.")}
    del outs, res, xin, m
    gc.collect()
    torch.cuda.empty_cache()
    return out


@pytest.fixture(scope="module")
def oracle_run():
    """run(name): the configuration's forward and oracle, computed once; one configuration is held at a time"""
    held = {}

    def get(name):
        if name not in held:
            held.clear()
            gc.collect()
            torch.cuda.empty_cache()
            held[name] = _run(name)
        return held[name]
    yield get
    held.clear()


def _limits(k):
    return (BLOCK0_MAX, BLOCK0_L2, BLOCK0_IMG_MAX) if k == 0 else (BLOCK_MAX, BLOCK_L2, BLOCK_IMG_MAX)


# ====================================================================================================================
# A-E per configuration: one parametrized test in configuration order, so that each configuration is computed once
# ====================================================================================================================

def check_elementwise(run):
    bl = run["blocks"]
    assert len(bl) == 33
    for sel, what in ((bl[:1], "block 0"), (bl[1:], "blocks 1-32")):
        for key in ("max", "l2", "img"):
            w = max(sel, key=lambda b: b[key])
            print(f"MEASURE A {run['name']} {what} worst {key}: {w[key]:.2e} ({w['name']})")
    bad = []
    for b in bl:
        lim_mx, lim_l2, lim_img = _limits(b["k"])
        if not (b["max"] < lim_mx and b["l2"] < lim_l2 and b["img"] < lim_img):
            img, y, x, c = b["at"]
            bad.append(f"block {b['k']} ({b['name']}): max-rel {b['max']:.2e}, L2 {b['l2']:.2e}, worst image {b['img_at']} at "
                       f"{b['img']:.2e}; largest error at (image, row, column, channel) = ({img}, {y}, {x}, {c})")
    assert not bad, f"{run['name']}:\n  " + "\n  ".join(bad)


def check_channel_moments(run):
    bl = run["blocks"]
    for key in ("mean", "std"):
        w = max(bl, key=lambda b: b[key])
        print(f"MEASURE B {run['name']} worst {key}: {w[key]:.2e} ({w['name']} channel {w[key + '_ch']})")
    bad = [f"block {b['k']} ({b['name']}): mean {b['mean']:.2e} (channel {b['mean_ch']}), std {b['std']:.2e} (channel {b['std_ch']})"
           for b in bl if not (b["mean"] < MOMENT_MEAN and b["std"] < MOMENT_STD)]
    assert not bad, f"{run['name']}:\n  " + "\n  ".join(bad)


def check_running_buffers(run):
    before, after, orc = run["before"], run["after"], run["oracle"]
    assert len(BNS) == 104
    if not run["cfg"]["train"]:     # eval: nothing moves
        for k, v in before.items():
            assert torch.equal(after[k], v), k
        return
    wm, wv, bad = (0.0, ""), (0.0, ""), []
    for bn in BNS:
        assert int(after[bn + ".num_batches_tracked"]) == 1, bn
        mg, vg = _batch_stats(after, before, bn)
        mo, vo = _batch_stats(orc, before, bn, 0.9, 0.1)
        em = ((mg - mo).abs() / vo.sqrt()).max().item()
        ev = (vg / vo - 1).abs().max().item()
        wm, wv = max(wm, (em, bn)), max(wv, (ev, bn))
        if not (em < RUN_MEAN and ev < RUN_VAR):
            bad.append(f"{bn}: batch mean {em:.2e} of std, unbiased variance {ev:.2e} relative")
    print(f"MEASURE C {run['name']}: batch mean {wm[0]:.2e} ({wm[1]}), variance {wv[0]:.2e} ({wv[1]})")
    assert not bad, f"{run['name']}:\n  " + "\n  ".join(bad)


def check_pooled(run):
    print(f"MEASURE D {run['name']}: pooled {run['pool']:.2e}")
    assert run["pool"] < POOL_MAX


def check_attention_map(run):
    """cnn_attn.ResNet's (B, 2048, 49) fp32 output is the last tap, channels first and widened to fp32, bit for bit"""
    assert run["ncp_exact"]


# ====================================================================================================================
# E. bench.py's pipelined route: three forwards in flight on their own workspaces, updates in minibatch order
# ====================================================================================================================

def _trainer(cnn, V=1000):
    from showtell_amd import optim
    from showtell_amd.rnn import RNN
    from showtell_amd.train import Trainer
    rnn = RNN(512, 512, V, 1, dtype=torch.bfloat16).cuda().train()
    opt = optim.SGD(Trainer.trainable_params(cnn, rnn), lr=0.01, momentum=0.9)
    return Trainer(cnn, rnn, opt)


def check_pipelined(run):
    """The image is the same every step, so after n steps every layer holds rm_n = a rm_0 + (1 - a) mean and
    rv_n = a rv_0 + (1 - a) var_unbiased with a = 0.9^n; mean and var_unbiased are C's oracle statistics."""
    n, V = 5, 1000
    B = run["cfg"]["B"]
    cnn = _model(run["params"], False, True)
    tr = _trainer(cnn, V)
    image = run["image"].cuda()
    cap, lens = R.synthetic_captions(B, V, seed=5)
    cap = cap.cuda()

    def ahead(k):      # bench.py's ahead(k, n)
        return dict(upcoming=[image] * min(tr.depth, n - 1 - k))
    for k in range(n):
        tr.step(image, cap, lens, **ahead(k))
    tr.flush()
    torch.cuda.synchronize()
    got, before, orc = _buffers(cnn), run["before"], run["oracle"]
    a32 = float(np.float32(KEEP32) ** n)
    wm = wv = 0.0
    bad = []
    for bn in BNS:
        assert int(got[bn + ".num_batches_tracked"]) == n, (bn, int(got[bn + ".num_batches_tracked"]))
        mg, vg = _batch_stats(got, before, bn, a32, 1.0 - a32)
        mo, vo = _batch_stats(orc, before, bn, 0.9, 0.1)
        em = ((mg - mo).abs() / vo.sqrt()).max().item()
        ev = (vg / vo - 1).abs().max().item()
        wm, wv = max(wm, em), max(wv, ev)
        if not (em < PIPE_MEAN and ev < PIPE_VAR):
            bad.append(f"{bn}: mean {em:.2e} of std, variance {ev:.2e} relative")
    print(f"MEASURE E: after {n} pipelined steps: batch mean {wm:.2e}, variance {wv:.2e}")
    assert not bad, "\n  ".join(bad)


CHECKS = {"A": check_elementwise, "B": check_channel_moments, "C": check_running_buffers, "D": check_pooled,
          "E": check_pipelined, "map": check_attention_map}
PLAN = {"b128": "A B C D E", "b127": "A B C D", "attn64": "A B C D map", "eval256": "A C D"}


@pytest.mark.parametrize("name,check", [(n, c) for n, cs in PLAN.items() for c in cs.split()],
                         ids=[f"{n}-{c}" for n, cs in PLAN.items() for c in cs.split()])
def test_encoder_bench_shape_matches_fp64_oracle(oracle_run, name, check):
    CHECKS[check](oracle_run(name))


# ====================================================================================================================
# F. prefetched forwards that the Trainer drops take their running-buffer updates with them
# ====================================================================================================================

def _drop_run(schedule):
    """ResNet-50 at 128 x 128, B = 16, as test_gpu_fullsize.test_pipelined_steps_equal_plain_steps.  `schedule`: (batch,
    upcoming batches, train mode) per step; an upcoming entry "k'" is a fresh copy of batch k's images (a list rebuilt every
    step).  Batch i's images are scaled and shifted by i, so that every batch leaves different statistics."""
    from showtell_amd.cnn import ResNet
    from showtell_amd.train import synthetic_batch
    E, V, B = 256, 1000, 16
    torch.manual_seed(7)
    cnn = ResNet(50, E, dtype=torch.bfloat16).cuda().train()
    tr = _trainer_small(cnn, E, V)
    batches = []
    for i in range(5):
        img, cap, lens = synthetic_batch(B, V, seed=20 + i, image_size=128)
        batches.append((img * (1.0 + 0.25 * i) + 0.2 * i, cap, lens))
    for i, ups, train in schedule:
        cnn.train(train)
        up = [batches[int(u[0])][0].clone() if u.endswith("'") else batches[int(u)][0] for u in ups]
        tr.step(*batches[i], upcoming=up)
    tr.flush()
    torch.cuda.synchronize()
    return _buffers(cnn)


def _trainer_small(cnn, E, V):
    from showtell_amd import optim
    from showtell_amd.rnn import RNN
    from showtell_amd.train import Trainer
    rnn = RNN(E, E, V, 2, dtype=torch.bfloat16).cuda().train()
    return Trainer(cnn, rnn, optim.SGD(Trainer.trainable_params(cnn, rnn), lr=0.05, momentum=0.9))


def _plain(schedule):
    return [(i, [], train) for i, _, train in schedule]


T, EV = True, False
DROPS = {
    # step(A, upcoming=[B]); step(C): _backbone meets an unexpected batch and drops B
    "backbone": ([(0, ["1"], T), (2, [], T)], None),
    # step(B) takes its prefetched forward, then upcoming=[C] disagrees with the prefetched D: step drops D
    "step": ([(0, ["1", "3"], T), (1, ["2"], T), (2, [], T)], None),
    # an upcoming list rebuilt every step with new tensor objects: every prefetch is dropped
    "rebuilt": ([(0, ["1'"], T), (1, ["2'"], T), (2, [], T)], None),
    # the dropped run starts with an eval-mode forward (no update) and ends with a train-mode one (an update): B and C are
    # prefetched in eval mode, B is taken, D is prefetched in train mode, step(E) drops C and D.  Every forward that ran is
    # the plain loop's in the same mode: A and B in eval mode, E in train mode
    "modes": ([(0, ["1", "2"], EV), (1, ["2", "3"], T), (4, [], T)], [(0, [], EV), (1, [], EV), (4, [], T)]),
}


@pytest.mark.parametrize("case,schedule", [(c, s) for c, (s, _) in DROPS.items()])
def test_dropped_prefetches_leave_the_running_buffers_alone(case, schedule):
    plain_schedule = DROPS[case][1] or _plain(schedule)
    plain = _drop_run(plain_schedule)
    got = _drop_run(schedule)
    bns = [k[:-len(".num_batches_tracked")] for k in plain if k.endswith(".num_batches_tracked")]
    want = sum(train for *_, train in plain_schedule)
    assert {int(plain[bn + ".num_batches_tracked"]) for bn in bns} == {want}
    nbt = {int(got[bn + ".num_batches_tracked"]) for bn in bns}
    assert nbt == {want}, f"{case}: num_batches_tracked {sorted(nbt)}, the plain loop {want}"
    wm = wv = 0.0
    for bn in bns:
        rv = plain[bn + ".running_var"].double()
        em = ((got[bn + ".running_mean"].double() - plain[bn + ".running_mean"].double()).abs() / rv.sqrt()).max().item()
        ev = ((got[bn + ".running_var"].double() - rv).abs() / rv).max().item()
        wm, wv = max(wm, em), max(wv, ev)
    print(f"MEASURE F {case}: running_mean {wm:.2e} of sqrt(running_var), running_var {wv:.2e} relative")
    assert wm < DROP_MEAN and wv < DROP_VAR, (case, wm, wv)


def test_encoder_state_dict_saves_after_a_forward():
    """The BatchNorm tensors are views into the engine's flat arrays once a forward ran: torch.save of the state dict as it
    stands (the reference's checkpoint code saves cnn.state_dict() directly) must work and load back exactly, also after a
    pipelined step that dropped a prefetched forward."""
    import io
    from showtell_amd.cnn import ResNet
    from showtell_amd.train import synthetic_batch
    E, V = 64, 1000
    cnn = ResNet(50, E, dtype=torch.bfloat16).cuda().train()
    tr = _trainer_small(cnn, E, V)
    batches = [synthetic_batch(4, V, seed=40 + i, image_size=64) for i in range(2)]
    tr.step(*batches[0], upcoming=[batches[1][0]])
    tr.step(*batches[0])                          # batch 1's prefetched forward is dropped
    tr.flush()
    torch.cuda.synchronize()
    sd = cnn.state_dict()
    f = io.BytesIO()
    torch.save({"encoder_state_dict": sd}, f)
    f.seek(0)
    back = torch.load(f, map_location="cpu")["encoder_state_dict"]
    assert back.keys() == sd.keys()
    for k, v in sd.items():
        assert back[k].dtype == v.dtype and torch.equal(back[k], v.cpu()), k
    assert int(back["model.1.num_batches_tracked"]) == 2
    fresh = ResNet(50, E, dtype=torch.bfloat16)
    fresh.load_state_dict(back)
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, back[k]), k
