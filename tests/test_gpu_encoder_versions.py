"""ResNet-18, -34, -50 and -152 at 224 x 224, block by block against the float64 oracle: the walk of
tests/test_gpu_encoder_bench_shape.py (which holds ResNet-101 to it) for every other version the encoder accepts.

The basic-block nets (18, 34) take a planner branch of their own and launch geometries nothing else reaches: 3 x 3 stride-2
convolutions with cin != cout and the generic stem on st_conv, 1 x 1 stride-2 downsample convolutions from 56 x 56, 28 x 28 and
14 x 14, a stand-alone "bn + identity + relu" whose identity carries a BatchNorm of its own with another replica count, and
in eval mode st_conv's "conv + residual" epilogue at every map size.  ResNet-152 is the longest chain the executor sees: 50
blocks, 155 BatchNorm layers, 160 train-mode launches.

Configurations (one forward with taps each, computed once by the module-scoped fixture, one held at a time):
  r<v>-train    bf16, B = 5, train: an odd image count, 245 samples per channel in layer4's statistics, every 112- and 128-row
                tile grid at 7 x 7 and 14 x 14 ends in a partial tile
  r<v>-eval     bf16, B = 3, eval
  r34-b64       bf16, B = 64, train: st_conv's stride-2 convolutions and the generic stem write more than one statistics replica
  r34-f32-*     fp32, B = 5 train / B = 3 eval: the basic-block branch on st_conv alone
ResNet-34 and -152 run through cnn_attn.ResNet (the map check), the others through cnn.ResNet; ResNet-34's head is checked on
cnn.ResNet.  For B = 5 / 3 the host-only plan must route every launch line to the kernel family B = 4 / 2 has (the batch sizes
the bounds of A were set at); B = 64 must have (replicas out, replicas in) pairs that B = 5 lacks.

Inputs and walk as in the bench-shape file: conv weights and images rounded to bf16, BatchNorm gains in [0.75, 1.25], random
biases and running buffers, undamped; stem + pool + block 0 from the image, block k from the HIP path's own tap k - 1.

A    every block output elementwise: max-rel, L2 and the worst per-image max-rel
C    running buffers of every BatchNorm layer: the absorbed batch mean and unbiased variance and num_batches_tracked == 1
     (train), bit-unchanged (eval)
D    pooled features against a float64 mean of the last tap
map  cnn_attn.ResNet's (B, F, 49) fp32 output is the last tap, channels first and widened, bit for bit
head cnn(image) against Linear -> BatchNorm1d(momentum 0.01) in float64 on the same forward's pooled features as the bf16 head
     stores them (F_in = 512)
log  a fresh process logs its launches (ST_LAYER_LOG); the host-only plan must give the same lines

tests/test_encoder_versions_inputs.py shows, without a GPU, that the reference alone stays within these bounds and that six
seeded faults do not.  The worst values measured on the MI355X are written next to each bound.
tests/test_gpu_encoder_sizes.py runs the same walk and checks at other image sizes (_run with a configuration of its own, the
check_* functions with the bounds it passes).
"""
import gc
import os
import subprocess
import sys

import pytest
import torch

from oracle import restatement as R
from tests._encoder_walk import (_bf16, _block_metrics, _blocks, _buffer_errors, _double, _nchw64, _params, _running,
                                 _stem_pool)
from tests.test_gpu_decoder_bench_shape import GRAD_L2, GRAD_MAX, _rel_l2, _rel_max
from tests.test_gpu_encoder import TOL, UNDAMPED_BLOCK, UNDAMPED_BLOCK0
from tests.test_gpu_encoder_bench_shape import (BLOCK0_IMG_MAX, BLOCK0_L2, BLOCK0_MAX, BLOCK_IMG_MAX, BLOCK_L2, BLOCK_MAX,
                                                POOL_MAX, RUN_MEAN, RUN_VAR)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16, F32 = torch.bfloat16, torch.float32
SMALL_B = {True: 4, False: 2}      # the batch sizes test_resnet101_bf16_block_by_block_undamped's bounds were set at


def _cfg(version, B, train, dtype=BF16, seed=0, head=False, H=224, W=224, attn=None):
    attn = (version in (34, 152) and dtype == BF16) if attn is None else attn
    return dict(version=version, B=B, train=train, dtype=dtype, attn=attn, head=head, seed=seed, H=H, W=W)


CONFIGS = {
    "r18-train": _cfg(18, 5, True, seed=51), "r18-eval": _cfg(18, 3, False, seed=52),
    "r34-train": _cfg(34, 5, True, seed=53, head=True), "r34-eval": _cfg(34, 3, False, seed=54, head=True),
    "r50-train": _cfg(50, 5, True, seed=55), "r50-eval": _cfg(50, 3, False, seed=56),
    "r152-train": _cfg(152, 5, True, seed=57), "r152-eval": _cfg(152, 3, False, seed=58),
    "r34-b64": _cfg(34, 64, True, seed=59),
    "r34-f32-train": _cfg(34, 5, True, F32, seed=60), "r34-f32-eval": _cfg(34, 3, False, F32, seed=61),
}

# A, bf16 at B = 5 / 3: test_resnet101_bf16_block_by_block_undamped's bounds (set on the same kernels at B = 4 / 2, three storage
# roundings per block; a basic block has two); per image, the bench-shape bounds widened by the same ratio.
# (max-rel, L2, worst per-image max-rel)
_RATIO = UNDAMPED_BLOCK[0] / BLOCK_MAX
SMALL = dict(
    # train 6.9e-3 (r152 layer3.0) / 4.7e-3 (r152 layer4.0) / 7.6e-3 (r152 layer3.0); eval 5.7e-3 / 2.8e-3 / 5.7e-3 (r50 layer2.0)
    block=(*UNDAMPED_BLOCK, BLOCK_IMG_MAX * _RATIO),
    # train 1.0e-2 / 1.0e-2 / 1.1e-2 (r152; r18 and r34: 7.4e-3 / 5.5e-3 / 8.3e-3); eval 5.5e-3 / 3.1e-3 / 5.5e-3 (r50)
    block0=(*UNDAMPED_BLOCK0, BLOCK0_IMG_MAX * _RATIO))
# A, ResNet-34 at B = 64: the bench-shape constants as they are
BENCH = dict(block=(BLOCK_MAX, BLOCK_L2, BLOCK_IMG_MAX),        # 6.9e-3 / 3.9e-3 / 6.9e-3 (layer2.0)
             block0=(BLOCK0_MAX, BLOCK0_L2, BLOCK0_IMG_MAX))    # 7.8e-3 / 5.2e-3 / 8.8e-3
# A, fp32: the project's fp32 bound for 104 layers, which one block must sit far below
FP32 = dict(block=(TOL[F32],) * 3, block0=(TOL[F32],) * 3)      # 1.8e-6 (eval layer4.0), block 0: 1.3e-6
# C: the bench-shape constants (measured there at 3 k - 12 k samples per channel in layer4), but for the variance at B = 5, where
# layer4 has 245 samples per channel: the variance of 245 values stored in bf16 against that of the unrounded ones.  Measured on
# the MI355X against the float64 oracle, worst of the five B = 5 configurations: 2.73e-3 (tests/test_encoder_versions_inputs.py:
# the reference alone, stored in bf16, 1.7e-3); the bound is twice that
BUFFER_MEAN = RUN_MEAN
BUFFER_VAR = {"small": 5.5e-3, "bench": RUN_VAR}
# ... which is above 1 / 245 = 4.1e-3, what a biased variance is short by.  So C also bounds the MEAN over a layer's channels of
# variance / oracle's - 1: rounding errors of the channels are independent and each below BUFFER_VAR, so their mean over C >= 64
# channels stays below BUFFER_VAR / sqrt(64) (generous: a bound on the worst channel stands in for their standard deviation); a
# wrong count moves every channel alike
VAR_OFFSET = {k: v / 8 for k, v in BUFFER_VAR.items()}
# D: POOL_MAX for bf16 taps (sums of 8-bit mantissas are all but exact in fp32).  fp32 taps: the a-priori bound of an fp32 sum
# of 49 non-negative values in any order, (n - 1) roundings of 2^-24, and one more for the division
POOL_MAX_F32 = 49 * 2.0 ** -24


def limits(cfg):
    """{'block': (max-rel, L2, per-image), 'block0': ...} of a configuration"""
    if cfg["dtype"] == F32:
        return FP32
    return SMALL if cfg["B"] <= 5 else BENCH


def buffer_limits(cfg):
    """C: (batch mean, variance per channel, variance offset of the layer)"""
    k = "small" if cfg["B"] <= 5 else "bench"
    return BUFFER_MEAN, BUFFER_VAR[k], VAR_OFFSET[k]


# ====================================================================================================================
# the plan: B = 5 / 3 keep the kernel routes of B = 4 / 2; ResNet-34 at B = 64 adds replica flows
# ====================================================================================================================

def _plan(cfg, B=None):
    from tests.test_resnet_plan import plan
    return plan(cfg["version"], "bf16" if cfg["dtype"] == BF16 else "f32", cfg["H"], cfg["W"], B or cfg["B"], cfg["train"])


def _replica_pairs(lines):
    from tests.test_resnet_plan import fields
    return {(fields(x)["rep_out"], fields(x)["rep_in"]) for x in lines}


def check_plan(name):
    from tests.test_resnet_plan import fields
    cfg = CONFIGS[name]
    if name == "r34-b64":
        new = _replica_pairs(_plan(cfg)) - _replica_pairs(_plan(CONFIGS["r34-train"]))
        assert new, "ResNet-34 at B = 64 moves statistics replicas as B = 5 does: pick the smallest B that does not"
        return
    a, b = _plan(cfg, SMALL_B[cfg["train"]]), _plan(cfg)
    assert len(a) == len(b) and all(fields(x)["family"] == fields(y)["family"] for x, y in zip(a, b)), \
        f"{name}: B = {cfg['B']} changes a kernel route against B = {SMALL_B[cfg['train']]}"


# ====================================================================================================================
# one forward with taps and its oracle
# ====================================================================================================================

def _model(cfg, params, attn):
    from showtell_amd.cnn import ResNet
    from showtell_amd.cnn_attn import ResNet as ResNetAttn
    m = (ResNetAttn if attn else ResNet)(cfg["version"], 512, dtype=cfg["dtype"])
    m.load_state_dict(params)
    return m.cuda().train(cfg["train"])


def _buffers(m):
    return {k: v.detach().cpu().clone() for k, v in _running(m.state_dict()).items()}


def _head(cfg, params, image):
    """cnn.ResNet's forward, the pooled features of the same forward, and the head's BatchNorm1d buffers around it"""
    g = torch.Generator().manual_seed(cfg["seed"] + 200)
    p = dict(params)
    p["linear_secondlast_layer.weight"] = _bf16(p["linear_secondlast_layer.weight"])
    p["last_layer.weight"] = torch.rand(512, generator=g) + 0.5
    p["last_layer.bias"] = torch.randn(512, generator=g) * 0.1
    m = _model(cfg, p, False)
    seen = []
    features = m.backbone_features
    m.backbone_features = lambda x, undo=None: (seen.append(features(x, undo=undo)), seen[-1])[1]
    y = m(image.cuda())
    torch.cuda.synchronize()
    assert len(seen) == 1
    bn = m.last_layer
    return dict(params=p, y=y.detach().cpu(), pooled=seen[0].cpu(), rm=bn.running_mean.cpu().clone(),
                rv=bn.running_var.cpu().clone(), nbt=int(bn.num_batches_tracked))


def _run(name, cfg=None):
    """One forward with taps of CONFIGS[name], or of `cfg` (tests/test_gpu_encoder_sizes.py: other image sizes), walked block by
    block against the oracle"""
    if cfg is None:
        cfg = CONFIGS[name]
        check_plan(name)
    v, B, train, attn = cfg["version"], cfg["B"], cfg["train"], cfg["attn"]
    params = _params(cfg["seed"], v)
    image = _bf16(torch.randn(B, 3, cfg["H"], cfg["W"], generator=torch.Generator().manual_seed(cfg["seed"])))
    m = _model(cfg, params, attn)
    before = _buffers(m)
    res = m._bb.block_outputs(image.cuda(), train, want_ncp=attn)
    outs, pooled = res[0], res[1].cpu()
    after = _buffers(m)
    out = dict(name=name, cfg=cfg, before=before, after=after, bns=[bn for *_, bn in R.resnet_conv_list(v)])
    blocks = _blocks(v)
    assert len(outs) == len(blocks) == sum(R.RESNET_SPECS[v][1])
    feat = outs[-1].shape[3]
    assert feat == (512 if R.RESNET_SPECS[v][0] == "basic" else 2048) and pooled.shape == (B, feat)
    out["tap_shapes"] = [tuple(o.shape) for o in outs]
    pixels = outs[-1].shape[1] * outs[-1].shape[2]       # 49 at 224 x 224
    if attn:
        out["ncp_shape"] = tuple(res[2].shape)
        out["ncp_exact"] = res[2].shape == (B, feat, pixels) and res[2].dtype == F32 and \
            torch.equal(res[2], outs[-1].float().permute(0, 3, 1, 2).reshape(B, feat, pixels))
    p = _double(params)
    mets = []
    with torch.no_grad():
        xin = _stem_pool(p, image.double(), train)
        for k, li, bi, bname in blocks:
            ref = R.block_forward(p, xin, v, li, bi, train)
            got = _nchw64(outs[k].cpu())
            assert got.shape == ref.shape, (k, got.shape, ref.shape)
            met = _block_metrics(got, ref, moments=False)
            met.update(k=k, name=bname)
            mets.append(met)
            del ref, xin
            xin = got
        pref = xin.mean((2, 3))
        out["pool"] = ((pooled.double() - pref).abs().max() / pref.abs().max()).item()
    out["blocks"] = mets
    out["oracle"] = _running(p)
    del outs, res, xin, m
    if cfg["head"]:
        out["head"] = _head(cfg, params, image)
    gc.collect()
    torch.cuda.empty_cache()
    return out


_stopped = []       # the configuration whose forward raised, or whose child process died: no later GPU work is started


def holder(run, stopped):
    """A module-scoped fixture's body: get(name) computes run(name) once and holds one configuration at a time; after a
    RuntimeError from the engine nothing more is started (`stopped`, the module's own list)."""
    held = {}

    def get(name):
        assert not stopped, f"not run: {stopped[0]} raised in the engine or died"
        if name not in held:
            held.clear()
            gc.collect()
            torch.cuda.empty_cache()
            try:
                held[name] = run(name)
            except RuntimeError:        # an engine or HIP error: nothing more is started on the GPU from this module
                stopped.append(name)
                raise
        return held[name]
    yield get
    held.clear()


@pytest.fixture(scope="module")
def oracle_run():
    yield from holder(_run, _stopped)


# ====================================================================================================================
# the checks (tests/test_encoder_versions_inputs.py applies A and C to a CPU emulation of bf16 storage)
# ====================================================================================================================

def failures_elementwise(run, lim=None):
    """A: the blocks beyond their bounds, as text.  lim: {'block': ..., 'block0': ...}; by default limits() of the configuration"""
    lim = lim or limits(run["cfg"])
    bad = []
    for b in run["blocks"]:
        lim_mx, lim_l2, lim_img = lim["block0" if b["k"] == 0 else "block"]
        if not (b["max"] < lim_mx and b["l2"] < lim_l2 and b["img"] < lim_img):
            img, y, x, c = b["at"]
            bad.append(f"block {b['k']} ({b['name']}): max-rel {b['max']:.2e}, L2 {b['l2']:.2e}, worst image {b['img_at']} at "
                       f"{b['img']:.2e}; largest error at (image, row, column, channel) = ({img}, {y}, {x}, {c})")
    return bad


def check_elementwise(run, lim=None):
    bl = run["blocks"]
    for sel, what in ((bl[:1], "block 0"), (bl[1:], f"blocks 1-{len(bl) - 1}")):
        for key in ("max", "l2", "img"):
            w = max(sel, key=lambda b: b[key])
            print(f"MEASURE A {run['name']} {what} worst {key}: {w[key]:.2e} ({w['name']})")
    bad = failures_elementwise(run, lim)
    assert not bad, f"{run['name']}:\n  " + "\n  ".join(bad)


def failures_running_buffers(run, bounds=None):
    """C (train): (layers beyond their bounds as text, then (worst error, layer) of the batch mean, the variance and the
    variance offset).  bounds: (mean, variance, offset); by default buffer_limits() of the configuration"""
    before, after, orc = run["before"], run["after"], run["oracle"]
    mean_bound, var_bound, off_bound = bounds or buffer_limits(run["cfg"])
    wm, wv, wo, bad = (0.0, ""), (0.0, ""), (0.0, ""), []
    for bn in run["bns"]:
        if int(after[bn + ".num_batches_tracked"]) != int(before[bn + ".num_batches_tracked"]) + 1:
            bad.append(f"{bn}: num_batches_tracked {int(after[bn + '.num_batches_tracked'])}")
        em, ev, eo = _buffer_errors(after, before, orc, bn)
        wm, wv, wo = max(wm, (em, bn)), max(wv, (ev, bn)), max(wo, (eo, bn))
        if not (em < mean_bound and ev < var_bound and eo < off_bound):
            bad.append(f"{bn}: batch mean {em:.2e} of std, unbiased variance {ev:.2e} relative, offset over the channels {eo:.2e}")
    return bad, wm, wv, wo


def check_running_buffers(run, bounds=None):
    before, after = run["before"], run["after"]
    assert len(run["bns"]) * 3 == len(before) == len(after)
    if not run["cfg"]["train"]:     # eval: nothing moves
        for k, v in before.items():
            assert torch.equal(after[k], v), k
        print(f"MEASURE C {run['name']}: {len(before)} buffers bit-unchanged")
        return
    assert all(int(before[bn + ".num_batches_tracked"]) == 0 for bn in run["bns"])
    bad, wm, wv, wo = failures_running_buffers(run, bounds)
    print(f"MEASURE C {run['name']}: batch mean {wm[0]:.2e} ({wm[1]}), variance {wv[0]:.2e} ({wv[1]}), "
          f"variance offset {wo[0]:.2e} ({wo[1]})")
    assert not bad, f"{run['name']}:\n  " + "\n  ".join(bad)


def check_pooled(run, bound=None):
    """bound: by default POOL_MAX (bf16 taps) or the a-priori bound of an fp32 sum over 49 pixels"""
    print(f"MEASURE D {run['name']}: pooled {run['pool']:.2e}")
    assert run["pool"] < (bound or (POOL_MAX_F32 if run["cfg"]["dtype"] == F32 else POOL_MAX))


def check_attention_map(run):
    print(f"MEASURE map {run['name']}: exact {run['ncp_exact']}")
    assert run["ncp_exact"]


def _head_oracle(h, x, train, mom=0.01):
    """Linear -> BatchNorm1d(momentum 0.01) in float64 on features x: (output, running mean, running variance)"""
    import torch.nn.functional as F
    p = h["params"]
    rm, rv = p["last_layer.running_mean"].double(), p["last_layer.running_var"].double()
    z = x @ p["linear_secondlast_layer.weight"].double().t() + p["linear_secondlast_layer.bias"].double()
    return F.batch_norm(z, rm, rv, p["last_layer.weight"].double(), p["last_layer.bias"].double(), train, mom, 1e-5), rm, rv


def check_head(run):
    """The head's output and, in train mode, the batch statistics its BatchNorm1d absorbed, with the bounds
    tests/test_gpu_decoder_bench_shape.py holds the bf16 head to (GRAD_L2, GRAD_MAX).  Those were set on features that are
    bf16 values, and the bf16 head stores its input in bf16 before anything else (head.py: ops.cast), so the oracle reads the
    same forward's pooled features rounded to bf16 -- as it reads bf16 images and filters.  Against the unrounded fp32 features
    the train-mode output is off by 1.4e-2 (L2) / 5.1e-2 (max): random images pool to nearly the same features (their spread
    over the batch is 0.14 of their mean), so BatchNorm1d over 5 samples magnifies that one input rounding; the float64 oracle
    on rounded against unrounded features shows the same 1.4e-2 / 5.3e-2 without any kernel.  That figure is printed, not
    asserted."""
    h, train, mom = run["head"], run["cfg"]["train"], 0.01
    p = h["params"]
    rm0, rv0 = p["last_layer.running_mean"].double(), p["last_layer.running_var"].double()
    ref, rm, rv = _head_oracle(h, _bf16(h["pooled"]).double(), train)
    raw = _head_oracle(h, h["pooled"].double(), train)[0]
    print(f"MEASURE head {run['name']} output against the oracle on unrounded features (not asserted): "
          f"rel_l2 {_rel_l2(h['y'], raw):.2e} rel_max {_rel_max(h['y'], raw):.2e}")
    res = {"output": (h["y"], ref)}
    if train:
        assert h["nbt"] == 1
        for key, got, r0, want in (("running_mean", h["rm"], rm0, rm), ("running_var", h["rv"], rv0, rv)):
            res["batch statistic of " + key] = ((got.double() - (1 - mom) * r0) / mom, (want - (1 - mom) * r0) / mom)
    else:
        assert h["nbt"] == 0 and torch.equal(h["rm"], p["last_layer.running_mean"]) and torch.equal(h["rv"], p["last_layer.running_var"])
    bad = []
    for what, (got, want) in res.items():
        l2, mx = _rel_l2(got, want), _rel_max(got, want)
        print(f"MEASURE head {run['name']} {what}: rel_l2 {l2:.2e} rel_max {mx:.2e}")
        if not (l2 < GRAD_L2 and mx < GRAD_MAX):
            bad.append((what, l2, mx))
    assert not bad, bad


CHECKS = {"A": check_elementwise, "C": check_running_buffers, "D": check_pooled, "map": check_attention_map, "head": check_head}
PLAN = {n: "A C D" + (" map" if c["attn"] else "") + (" head" if c["head"] else "") for n, c in CONFIGS.items()}


@pytest.mark.parametrize("name,check", [(n, c) for n, cs in PLAN.items() for c in cs.split()],
                         ids=[f"{n}-{c}" for n, cs in PLAN.items() for c in cs.split()])
def test_encoder_version_matches_fp64_oracle(oracle_run, name, check):
    CHECKS[check](oracle_run(name))


# ====================================================================================================================
# log: the executor launches what the planner says
# ====================================================================================================================

def check_launch_log(name, cfg, tmp_path, stopped):
    """One backbone_features in a fresh process with ST_LAYER_LOG set (the engine opens the log once per process), compared
    with st_resnet_plan's text line for line.  Each child runs under its own time limit; after a child that died or ran out of
    time no further child is started (`stopped`, the calling module's own list)."""
    assert not stopped, f"not started: {stopped[0]} raised in the engine or died"
    log = tmp_path / "launches.txt"
    cmd = [sys.executable, os.path.join(ROOT, "tests", "_layer_log_child.py"), str(cfg["version"]),
           "bf16" if cfg["dtype"] == BF16 else "f32", str(cfg["B"]), str(int(cfg["train"])), str(log), str(cfg["H"]), str(cfg["W"])]
    try:
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        stopped.append(name)
        raise
    if r.returncode != 0:
        stopped.append(name)
    assert r.returncode == 0, r.stderr[-2000:]
    got, want = log.read_text().splitlines(), _plan(cfg)
    assert len(got) == len(want), (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "launch %d" % i


@pytest.mark.parametrize("name", list(CONFIGS))
def test_executor_logs_what_the_planner_says(name, tmp_path):
    check_launch_log(name, CONFIGS[name], tmp_path, _stopped)
