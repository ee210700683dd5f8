"""The cases of tests/test_gpu_encoder_sizes.py (tests/_encoder_size_cases.py) without a GPU: they take the kernel routes they
are named for, the reference alone stays within their bounds, and seeded faults do not.

paths      from st_resnet_plan (host-only) alone: the generic stem and its reduction in the odd bottleneck cases, layer3's conv2
           on st_conv behind five reductions at 32 x 544, the 224 x 224 kernel families everywhere else, st_conv alone in fp32; the
           widest maps st_conv3x3_img takes; the refusal of H or W below 32
reference  tests/test_encoder_versions_inputs.Emulation (the float64 oracle with bf16 storage) on every bf16 case, walked and
           judged by the GPU file's own checks A, C and D with the cases' bounds.  It must pass, and in C its variance figure must
           stay below HALF the bound: BUFFER_VAR["small"] was set at 245 samples per channel, and storage rounding grows as the
           samples shrink, so the cases keep at least 480 samples per channel in layer4 (checked here too)
faults     seeded into the emulation of one block of these cases' own inputs; the named check must fail:
             zero-row     r101-wide, layer1.1 conv2, image 1: the last row of the last 2-row band of a 16 x 112 map     A per image
             b-minus-1    r50-min, a layer4 BatchNorm (1 x 1 map): 511 of 512 samples                                   C
             replica      r50-odd, the stem's BatchNorm: one of four replicas is left out                               C
             biased-var   r50-tall, layer4 (504 samples): short by 1 / 504 in every channel alike                       C (offset)
             pad-column   r50-odd, layer2.1 conv2 (9 x 57): the column beyond W reads the next row's first column      A
             pool-49      r50-tall (14 x 2 = 28 pixels) and r50-odd-eval (4 pixels): the mean divides by 49            D

Figures of the emulation, from this file's MEASURE lines (seeds of the cases):
  C variance, worst channel over the seven bf16 train cases   1.2e-3 - 1.8e-3 (worst r50-fallback, model.7.0.bn3)   bound 5.5e-3, half 2.75e-3
  C batch mean                                                at most 7.8e-4 (r50-fallback)                          bound 4e-3
  C variance offset                                           at most 5.2e-5 (r50-min)                               bound 6.9e-4
  A train, worst block (layer1.0): max-rel / L2 / per image   at most 8.8e-3 / 8.3e-3 / 1.3e-2 (r50-min per image)   3e-2 / 2e-2 / 5e-2
  A eval, worst block: max-rel / L2 / per image               at most 7.2e-3 / 3.7e-3 / 7.3e-3 (r101-p64 layer3.14)  2e-2 / 1e-2 / 2.7e-2
  D                                                           at most 6.3e-8                                         POOL_MAX
  faults: zero-row 4.5e-1 per image; pad-column max-rel 3.5e-1; b-minus-1 mean 6.7e-3, variance 2.1e-2; replica variance 2.5e-1;
  biased-var offset 2.00e-3 (1 / 504 = 1.98e-3); pool-49 4.3e-1 (28 pixels) and 9.2e-1 (4 pixels)

`python -m tests.test_encoder_sizes_inputs` prints the figures of every case."""
import collections

import pytest
import torch

from oracle import restatement as R
from tests import _encoder_size_cases as S
from tests._encoder_walk import _bf16, _blocks, _double, _params, _running
from tests.test_encoder_versions_inputs import Emulation, _block_index, _figures, _pool_error, _run_dict, clean, faulted
from tests.test_gpu_encoder_versions import SMALL_B, failures_elementwise, failures_running_buffers

BF16_CASES = [n for n, c in S.CASES.items() if c["dtype"] == S.BF16]
BOTTLENECK = [n for n in BF16_CASES if R.RESNET_SPECS[S.CASES[n]["version"]][0] == "bottleneck"]
# the blocks whose input tap the fault tests start from (the others are not kept)
FAULT_BLOCKS = {"r101-wide": ("layer1.1",), "r50-min": ("layer4.1",), "r50-odd": ("layer2.1",), "r50-tall": ("layer4.1",)}


# ====================================================================================================================
# paths
# ====================================================================================================================

def _lines(name, H=None, W=None, B=None):
    from tests.test_resnet_plan import fields, plan
    c = S.CASES[name]
    out = []
    for line in plan(c["version"], S.dtype_name(c), H or c["H"], W or c["W"], B or c["B"], c["train"]):
        f = fields(line)
        f["hin"], f["win"] = int(line.split(",")[6]), int(line.split(",")[7])
        out.append(f)
    return out


def _geo(f):
    return f["cin"], f["cout"], f["k"], f["stride"]


def _families(lines):
    return collections.Counter(f["family"] for f in lines)


@pytest.mark.parametrize("name", S.ODD_BOTTLENECK + ("r50-f32-odd",))
def test_an_odd_size_takes_the_generic_stem(name):
    lines = _lines(name)
    fam = _families(lines)
    assert "stem_pool" not in fam
    assert _geo(lines[0]) == (3, 64, 7, 2) and lines[0]["family"] == "igemm"
    red = [f for f in lines if f["family"] == "bn_reduce_replicas"]
    if name in S.ODD_BOTTLENECK:
        assert fam["igemm"] == 1
    else:
        assert set(fam) == {"igemm", "bn_act", "bn_reduce_replicas"} and fam["igemm"] == 53
    if S.CASES[name]["train"]:
        # st_conv keeps at least 128 tiles of 128 output pixels per statistics replica: two replicas from 32768 stem output pixels
        # on, four from 65536.  11 x 33 x 225 = 81675 pixels are 639 tiles: four replicas, reduced behind the stem (the pool reads
        # replica 0)
        c = S.CASES[name]
        tiles = (c["B"] * ((c["H"] - 1) // 2 + 1) * ((c["W"] - 1) // 2 + 1) + 127) // 128
        rep = max(r for r in (1, 2, 4, 8, 16, 32, 64) if r == 1 or tiles // r >= 128)
        assert rep == 4
        assert lines[0]["rep_out"] == rep and lines[1] is red[0] and len(red) == 1
        assert (red[0]["cout"], red[0]["rep_in"], red[0]["rep_out"]) == (64, rep, 1)
    else:
        assert not red
    if name in S.ODD_BOTTLENECK:    # and nothing else moves: the even neighbour differs by the stem's lines alone
        c = S.CASES[name]
        even = _families(_lines(name, c["H"] - 1, c["W"] - 1))
        assert fam - collections.Counter(igemm=1, bn_reduce_replicas=len(red)) == even - collections.Counter(stem_pool=1)


@pytest.mark.parametrize("name", S.FALLBACK)
def test_a_layer3_map_wider_than_33_falls_to_st_conv(name):
    lines = _lines(name)
    train = S.CASES[name]["train"]
    at = [i for i, f in enumerate(lines) if f["family"] == "igemm"]
    assert len(at) == 5 and all(_geo(lines[i]) == (256, 256, 3, 1) and (lines[i]["hin"], lines[i]["win"]) == (2, 34) for i in at)
    fam = _families(lines)
    assert fam["conv3x3_img"] == 8 and fam["bn_reduce_replicas"] == (5 if train else 0)
    for i in at:
        red = lines[i - 1]
        if train:       # st_conv's loader reads replica 0: conv1's four replicas are reduced in front of it
            assert (red["family"], red["cout"], red["rep_in"], red["rep_out"]) == ("bn_reduce_replicas", 256, 4, 1)
            assert lines[i]["rep_in"] == 1
        else:
            assert red["family"] != "bn_reduce_replicas"
    # one pixel narrower (layer3 33 wide), the same convolutions are st_conv3x3_img's and no reduction is left
    narrow = _families(_lines(name, W=S.CASES[name]["W"] - 16))
    assert narrow["conv3x3_img"] == 13 and "igemm" not in narrow and "bn_reduce_replicas" not in narrow


@pytest.mark.parametrize("name", [n for n in BOTTLENECK if n not in S.ODD_BOTTLENECK + S.FALLBACK])
def test_every_other_bottleneck_case_runs_the_kernel_families_of_224(name):
    assert _families(_lines(name)) == _families(_lines(name, 224, 224, SMALL_B[S.CASES[name]["train"]]))


def test_the_cases_reach_the_maps_they_are_named_for():
    def maps(name, family, cin=None):
        return {(f["hin"], f["win"]) for f in _lines(name) if f["family"] == family and cin in (None, f["cin"])}
    assert maps("r101-wide", "conv3x3_img", 64) == {(16, 112)} and (16, 112) in maps("r101-wide", "conv3x3_s2")
    assert maps("r50-tall", "conv3x3_img") == {(112, 16), (56, 8), (28, 4), (14, 2)}
    assert maps("r50-min", "conv3x3_img") == {(8, 8), (4, 4), (2, 2), (1, 1)}
    assert maps("r50-odd", "conv3x3_img") == {(17, 113), (9, 57), (5, 29), (3, 15)}
    assert maps("r50-odd", "conv3x3_s2") == {(17, 113), (9, 57), (5, 29)}
    assert maps("r101-p64", "conv3x3_img", 256) == {(16, 16)}
    assert maps("r18-wide-eval", "igemm") >= {(16, 112), (8, 56), (4, 28), (2, 14)}
    assert S.stage_maps(224, 224) == [(56, 56), (28, 28), (14, 14), (7, 7)]
    assert S.stage_maps(65, 449) == [(17, 113), (9, 57), (5, 29), (3, 15)] and S.stage_maps(32, 32)[3] == (1, 1)
    for name, c in S.TRAIN.items():
        assert S.layer4_samples(c) >= S.MIN_SAMPLES, name
    for c in S.CASES.values():          # the cost: at most 10.5 images of 224 x 224
        assert c["B"] * c["H"] * c["W"] <= 10.5 * 224 * 224


def test_the_widest_maps_of_conv3x3_img():
    from showtell_amd import ops
    for C, w in S.WIDEST.items():
        for h in (1, 2, 9):
            assert ops.conv3x3_img_supported(h, w, C, C) > 0, (C, w)
            assert ops.conv3x3_img_supported(h, w + 1, C, C) == 0, (C, w + 1)


@pytest.mark.parametrize("H,W", [(31, 64), (64, 31), (31, 31)])
def test_the_planner_refuses_an_image_below_32(H, W):
    from tests.test_resnet_plan import plan_refusal
    for train in (True, False):
        n, msg = plan_refusal(50, "bf16", H, W, 2, train)
        assert n == -1 and "bad arguments" in msg


# ====================================================================================================================
# the reference alone, and the faults
# ====================================================================================================================

def _args(name):
    c = S.CASES[name]
    keep = tuple(_block_index(c["version"], b) for b in FAULT_BLOCKS.get(name, ()))
    return (c["version"], c["train"]), dict(H=c["H"], W=c["W"], B=c["B"], seed=c["seed"], name=name, keep=keep)


def _clean(name):
    a, kw = _args(name)
    return clean(*a, **kw)


def _faulted(name, block, fault):
    a, kw = _args(name)
    return faulted(*a, _block_index(a[0], block), fault, **kw)


@pytest.mark.parametrize("name", BF16_CASES)
def test_the_reference_in_bf16_storage_stays_within_the_bounds_at_every_size(name):
    cfg = S.CASES[name]
    run = _clean(name)["run"]
    print("MEASURE", _figures(run), f"; D {run['pool']:.2e}")
    assert run["tap_shapes"] == S.tap_shapes(cfg)
    assert not failures_elementwise(run, S.limits(cfg))
    assert run["pool"] < S.pool_limit(cfg)
    if cfg["train"]:
        assert len(run["bns"]) == len(R.resnet_conv_list(cfg["version"]))
        bad, wm, wv, wo = failures_running_buffers(run, S.buffer_limits(cfg))
        assert not bad, bad
        assert wv[0] < S.buffer_limits(cfg)[1] / 2, wv


def test_a_zeroed_last_row_of_a_two_row_band_fails_the_per_image_check():
    run = _faulted("r101-wide", "layer1.1", ("zero-row", "model.4.1.conv2"))
    b = run["blocks"][0]
    print("MEASURE", _figures(run), "image", b["img_at"], "at", b["at"])
    lim_mx, lim_l2, lim_img = S.limits(run["cfg"])["block"]
    assert failures_elementwise(run, S.limits(run["cfg"]))
    assert b["img"] > lim_img and b["img_at"] == 1 and b["at"][0] == 1


def test_a_pad_column_read_from_the_next_row_fails_the_elementwise_check():
    run = _faulted("r50-odd", "layer2.1", ("pad-column", "model.5.1.conv2"))
    b = run["blocks"][0]
    print("MEASURE", _figures(run), "at", b["at"])
    assert failures_elementwise(run, S.limits(run["cfg"]))
    assert not failures_elementwise(_faulted("r50-odd", "layer2.1", None), S.limits(run["cfg"]))     # the block alone, clean


def _stem_faulted(name, fault):
    """the stem alone with `fault`: a run with no blocks whose only BatchNorm layer is the stem's"""
    c = S.CASES[name]
    params = _params(c["seed"], c["version"])
    image = _bf16(torch.randn(c["B"], 3, c["H"], c["W"], generator=torch.Generator().manual_seed(c["seed"]))).double()
    p, before = _double(params), {k: v.clone() for k, v in _running(params).items()}
    emu = Emulation(_double(params), True, fault)
    with torch.no_grad():
        R._bn2d(p, torch.nn.functional.conv2d(image, p["model.0.weight"], None, 2, 3), "model.1", True)
        emu.stem(image)
    return _run_dict(c, f"{name} stem {fault and fault[0]}", [], emu, before, p)


@pytest.mark.parametrize("name,block,kind,bn", [("r50-min", "layer4.1", "b-minus-1", "model.7.1.bn3"),
                                                ("r50-odd", "stem", "replica", "model.1"),
                                                ("r50-tall", "layer4.1", "biased-var", "model.7.1.bn2")])
def test_a_statistics_fault_fails_the_running_buffer_check_at_these_sizes(name, block, kind, bn):
    cfg = S.CASES[name]
    if block == "stem":
        clean_bad = failures_running_buffers(_stem_faulted(name, None), S.buffer_limits(cfg))[0]
        assert not clean_bad, clean_bad
        run = _stem_faulted(name, (kind, bn))
    else:
        run = _faulted(name, block, (kind, bn))
    bad, wm, wv, wo = failures_running_buffers(run, S.buffer_limits(cfg))
    print("MEASURE", run["name"], f"batch mean {wm[0]:.2e} ({wm[1]}), variance {wv[0]:.2e} ({wv[1]}), variance offset {wo[0]:.2e} ({wo[1]})")
    assert any(line.startswith(bn + ":") for line in bad), (bn, bad)
    if kind == "biased-var":
        # layer4 of r50-tall: 18 x 14 x 2 = 504 samples, every channel's variance is short by 1 / 504 = 1.98e-3: below the
        # per-channel bound, the offset over the channels sees it.  A clean run has |offset| < off_bound, so the biased one is
        # caught whenever 1 / n > 2 x off_bound (here 2.9 x; the 4 x of the 245-sample file cannot hold for any case that keeps
        # the 480 samples the variance bound needs: 1 / 480 = 3.0 x off_bound)
        n = S.layer4_samples(cfg)
        _, var_bound, off_bound = S.buffer_limits(cfg)
        assert n == 504 and 1 / n < var_bound and 1 / n > 2 * off_bound
        assert wo[1] == bn and abs(wo[0] - 1 / n) < off_bound / 4
        assert all(line.startswith(bn + ":") for line in bad), bad      # and nothing else moved


@pytest.mark.parametrize("name", ["r50-tall", "r50-odd-eval"])
def test_a_mean_over_49_pixels_fails_the_pooled_check(name):
    cfg = S.CASES[name]
    c = _clean(name)
    last = c["last"].double()
    emu = Emulation(None, cfg["train"], ("pool-49", None))
    err = _pool_error(emu.pool(last), last)
    print(f"MEASURE {name} pool-49: D {err:.2e} (clean {c['run']['pool']:.2e})")
    assert last.shape[2] * last.shape[3] != 49 and c["run"]["pool"] < S.pool_limit(cfg)
    assert err > S.pool_limit(cfg)


if __name__ == "__main__":
    for n in BF16_CASES:
        r = _clean(n)["run"]
        print(_figures(r), f"; D {r['pool']:.2e}")
