"""The encoder engine at image sizes other than 224 x 224, block by block against the float64 oracle: the walk of
tests/test_gpu_encoder_versions.py (its _run, its check_* and failures_* functions, its bounds) on the cases of
tests/_encoder_size_cases.py -- wide, tall, odd, smallest (32 x 32) and the 32 x 544 image whose layer3 no longer fits
st_conv3x3_img.  tests/test_encoder_sizes_inputs.py shows without a GPU that the cases take the routes they are named for, that the
reference alone stays within the bounds and that seeded faults do not.

One forward with taps per case (computed once by the module-scoped fixture, one held at a time), one test per (case, check):
A    every block output against R.block_forward in float64: max-rel, L2, worst per-image max-rel; the tap shapes are the map
     arithmetic of the cases file (and equal the oracle's)
C    train: the batch mean and unbiased variance each BatchNorm's running buffers absorbed, the variance offset over the channels,
     num_batches_tracked == 1; eval: buffers bit-unchanged
D    pooled features against the float64 mean of the last tap over its h * w pixels
map  cnn_attn.ResNet's (B, F, h * w) fp32 output is the last tap, channels first and widened, bit for bit
log  a fresh process logs its launches (ST_LAYER_LOG); st_resnet_plan for the same (version, dtype, H, W, B, train) gives the same
     lines
and two tests of the Python layer: the workspaces follow a shape change and leave the results bit-equal; H or W = 31 is refused.

After a RuntimeError from the engine, or a child that died or timed out, nothing more in this module starts GPU work (_stopped).

Bounds (none is new, tests/_encoder_size_cases.py) and the worst values measured on the MI355X:
  (A: max-rel, L2, worst per-image max-rel)
  A bf16 train  block 0    (3e-2, 2e-2, 5e-2)       1.06e-2 (r101-wide) / 1.02e-2 (r50-tall) / 1.56e-2 (r50-min)
                blocks 1-  (2e-2, 1e-2, 2.7e-2)     6.6e-3 (r50-tall layer2.0) / 4.7e-3 (r50-min layer4.0) / 9.9e-3 (r50-min layer2.0)
  A bf16 eval   block 0    (3e-2, 2e-2, 5e-2)       5.8e-3 / 3.5e-3 / 6.0e-3 (r152-p15)
                blocks 1-  (2e-2, 1e-2, 2.7e-2)     5.8e-3 (r50-fallback-eval layer4.0) / 2.7e-3 (r101-p64 layer4.0) / 5.8e-3
  A fp32        1e-3 each                           block 0: 7.3e-6 / 2.2e-6 / 8.4e-6; blocks 1-: 1.5e-6 / 1.2e-6 / 1.7e-6 (layer4.0)
  C batch mean  4e-3       1.83e-3 (r50-fallback model.4.0.downsample.1); fp32 3.4e-6
  C variance    5.5e-3     1.92e-3 (r101-wide model.7.0.bn3; the emulation alone: 1.77e-3); fp32 4.2e-5
  C offset      6.9e-4     2.7e-4 (r101-wide model.4.0.bn1); fp32 2.3e-7
  D bf16        2e-7       9.3e-8 (r34-mid)
  D fp32        45 x 2^-24 = 2.7e-6      2.7e-7
  eval buffers bit-unchanged, both maps bit-exact, eval at 224 x 224 bit-reproducible; every forward and log child under 4 s
"""
import pytest
import torch

from tests import _encoder_size_cases as S
from tests import test_gpu_encoder_versions as V
from tests._encoder_walk import _bf16, _params, _running

pytestmark = pytest.mark.gpu

_stopped = []       # the case whose forward raised, or whose child process died: no later GPU work is started


def _run(name):
    return V._run(name, S.CASES[name])


@pytest.fixture(scope="module")
def size_run():
    yield from V.holder(_run, _stopped)


def check_elementwise(run):
    assert run["tap_shapes"] == S.tap_shapes(run["cfg"])
    V.check_elementwise(run, S.limits(run["cfg"]))


def check_running_buffers(run):
    V.check_running_buffers(run, S.buffer_limits(run["cfg"]))


def check_pooled(run):
    V.check_pooled(run, S.pool_limit(run["cfg"]))


def check_attention_map(run):
    cfg = run["cfg"]
    h, w = S.stage_maps(cfg["H"], cfg["W"])[3]
    assert run["ncp_shape"] == (cfg["B"], 2048, h * w) and h * w != 49
    V.check_attention_map(run)


CHECKS = {"A": check_elementwise, "C": check_running_buffers, "D": check_pooled, "map": check_attention_map}
PLAN = {n: "A C D" + (" map" if c["attn"] else "") for n, c in S.CASES.items()}


@pytest.mark.parametrize("name,check", [(n, c) for n, cs in PLAN.items() for c in cs.split()],
                         ids=[f"{n}-{c}" for n, cs in PLAN.items() for c in cs.split()])
def test_encoder_matches_fp64_oracle_at_this_size(size_run, name, check):
    CHECKS[check](size_run(name))


@pytest.mark.parametrize("name", list(S.CASES))
def test_executor_logs_what_the_planner_says_at_this_size(name, tmp_path):
    V.check_launch_log(name, S.CASES[name], tmp_path, _stopped)


def _resnet50(seed, train):
    from showtell_amd.cnn import ResNet
    m = ResNet(50, 512, dtype=torch.bfloat16)
    m.load_state_dict(_params(seed, 50))
    return m.cuda().train(train)


def _images(B, H, W, seed):
    return _bf16(torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(seed))).cuda()


def test_workspaces_follow_a_shape_change_and_results_stay_bit_equal():
    """cnn.py keeps one workspace per (B, H, W, stream) and drops the others when the shape changes.  Eval, ResNet-50 bf16, B = 2,
    one module: 224 x 224 twice (bit-equal: eval is deterministic), 64 x 448, 33 x 33, 224 x 224 again (bit-equal to the first),
    and 64 x 448 on a fresh module (bit-equal to this module's): no slot size, pad column or statistics buffer of another shape
    leaks into a forward."""
    assert not _stopped, f"not run: {_stopped[0]} raised in the engine or died"
    try:
        m = _resnet50(96, False)
        before = {k: v.detach().cpu().clone() for k, v in _running(m.state_dict()).items()}
        x224, xwide, xodd = _images(2, 224, 224, 1), _images(2, 64, 448, 2), _images(2, 33, 33, 3)

        def shapes():
            return {k[1:4] for k in m._bb.ws}
        first = m.backbone_features(x224).clone()
        again = m.backbone_features(x224).clone()
        assert torch.equal(first, again), "eval mode is not deterministic at 224 x 224"
        assert shapes() == {(2, 224, 224)}
        wide = m.backbone_features(xwide).clone()
        assert shapes() == {(2, 64, 448)}
        odd = m.backbone_features(xodd).clone()
        assert shapes() == {(2, 33, 33)} and len(m._bb.ws) == 1
        back = m.backbone_features(x224).clone()
        assert shapes() == {(2, 224, 224)} and len(m._bb.ws) == 1
        assert torch.equal(back, first)
        fresh = _resnet50(96, False).backbone_features(xwide)
        torch.cuda.synchronize()
        assert torch.equal(fresh, wide)
        assert wide.shape == odd.shape == first.shape == (2, 2048) and bool(torch.isfinite(odd).all())
        assert not torch.equal(wide, first) and not torch.equal(odd, first)
        for k, v in _running(m.state_dict()).items():
            assert torch.equal(v.cpu(), before[k]), k
    except RuntimeError:
        _stopped.append("shape change")
        raise


@pytest.mark.parametrize("H,W", [(31, 64), (64, 31)])
def test_an_image_below_32_is_refused_and_nothing_is_launched(H, W):
    """H = 31 or W = 31: ShowTellHipError (unsupported input size) before the engine is called -- in train mode the running
    buffers and num_batches_tracked stay as they were and no workspace is kept -- and the planner refuses the same arguments."""
    from showtell_amd import ShowTellHipError
    from tests.test_resnet_plan import plan_refusal
    assert not _stopped, f"not run: {_stopped[0]} raised in the engine or died"
    m = _resnet50(97, True)
    try:
        m.backbone_features(_images(2, 32, 32, 4))          # a forward the engine accepts: weights packed, buffers flattened
        torch.cuda.synchronize()
    except RuntimeError:
        _stopped.append("refusal")
        raise
    before = {k: v.detach().cpu().clone() for k, v in _running(m.state_dict()).items()}
    held = dict(m._bb.ws)
    with pytest.raises(ShowTellHipError, match="unsupported input size"):
        m.backbone_features(_images(2, H, W, 5))
    torch.cuda.synchronize()
    assert m._bb.ws.keys() == held.keys()
    for k, v in _running(m.state_dict()).items():
        assert torch.equal(v.cpu(), before[k]), k
    assert all(int(v) == 1 for k, v in before.items() if k.endswith("num_batches_tracked"))
    n, msg = plan_refusal(50, "bf16", H, W, 2, True)
    assert n == -1 and "bad arguments" in msg
