"""The cases of tests/test_gpu_encoder_sizes.py (the encoder engine at image sizes other than 224 x 224) and of
tests/test_encoder_sizes_inputs.py (the same cases without a GPU): names, the map arithmetic, the bound selection.  A plain
module: no test lives here.

st_resnet_forward accepts every image with H, W >= 32.  What a size changes:
  - the maps: 8 x 8 down to 1 x 1 at 32 x 32; odd H or W gives odd maps at every stage (65 x 449: 17 x 113, 9 x 57, 5 x 29, 3 x 15)
  - odd H or W: no blocked-image stem.  The bottleneck nets then run the generic stem on st_conv and the stand-alone pool with
    bn1 folded in; from 32768 stem output pixels on the stem writes two statistics replicas and a reduction follows
  - wide maps: st_conv3x3_img forms bands of 16 * tm / (W + 2) rows and takes C = 64 up to W = 254, 128 up to 167, 256 up to 33,
    512 up to 40 (WIDEST); past that a 3 x 3 convolution falls to st_conv, in train mode with the producer's BatchNorm + ReLU in
    its loader behind a reduction of the producer's replicas (32 x 544: layer3 is 2 x 34)

Inputs as in tests/_encoder_walk.py: _params(seed, version), images rounded to bf16, undamped; block k of the oracle starts from
the HIP path's tap k - 1.

Bounds: none is new.  A and D take SMALL / POOL_MAX of tests/test_gpu_encoder_versions.py (fp32: FP32 and the a-priori sum bound
over h * w pixels), C takes BUFFER_MEAN, BUFFER_VAR["small"] and its offset.  BUFFER_VAR["small"] was set at 245 samples per
channel in layer4; rounding noise grows as the samples shrink (64 samples: the bf16-storage emulation alone reaches 6.1e-3), so
the rule is on the INPUTS: every train case has at least MIN_SAMPLES = 480 samples per channel in layer4, and
tests/test_encoder_sizes_inputs.py holds the emulation below half the variance bound."""
import torch

from tests.test_gpu_encoder_versions import (BUFFER_MEAN, BUFFER_VAR, FP32, POOL_MAX, SMALL, VAR_OFFSET, _cfg)

BF16, F32 = torch.bfloat16, torch.float32
MIN_SAMPLES = 480
# st_conv3x3_img's widest map per channel count (st_conv3x3_img_supported, H = 2)
WIDEST = {64: 254, 128: 167, 256: 33, 512: 40}


def _case(version, H, W, B, train, seed, dtype=BF16, attn=False):
    return _cfg(version, B, train, dtype, seed=seed, H=H, W=W, attn=attn)


TRAIN = {
    # maps 16 x 112 down to 2 x 14 on the benchmark net: conv3x3_img<64> in bands of 2 rows, conv3x3_s2 from 112 wide
    "r101-wide": _case(101, 64, 448, 18, True, 81),
    # 112 rows by 16 wide: many bands per image, W + 2 = 18 and 10
    "r50-tall": _case(50, 448, 64, 18, True, 82),
    # generic stem + folded pool + bn_reduce_replicas (64, 2) in a bottleneck net; odd maps at every stage
    "r50-odd": _case(50, 65, 449, 11, True, 83),
    # the smallest accepted size, 1 x 1 final map, 512 images on the grids' batch axis
    "r50-min": _case(50, 32, 32, 512, True, 84),
    # layer3's conv2 on st_conv with the producer's BatchNorm in its loader, five reductions; final map 1 x 17
    "r50-fallback": _case(50, 32, 544, 29, True, 85),
    # the basic-block branch at odd wide maps
    "r18-odd": _case(18, 65, 449, 11, True, 86),
    # non-square even maps 24 x 40 down to 3 x 5
    "r34-mid": _case(34, 96, 160, 33, True, 87),
    # the whole net on st_conv, 53 igemm launches, odd maps
    "r50-f32-odd": _case(50, 65, 449, 11, True, 88, dtype=F32),
}
EVAL = {
    # through cnn_attn: the map is (2, 2048, 64), the decoders' largest P; layer3 is 16 x 16, one workgroup per 14-row band
    "r101-p64": _case(101, 256, 256, 2, False, 91, attn=True),
    "r152-p15": _case(152, 96, 160, 3, False, 92, attn=True),          # P = 15
    "r50-odd-eval": _case(50, 33, 33, 3, False, 93),                   # generic stem; final map 2 x 2
    "r18-wide-eval": _case(18, 64, 448, 3, False, 94),                 # st_conv's residual epilogue on wide maps
    "r50-fallback-eval": _case(50, 32, 544, 3, False, 95),             # layer3's conv2 on st_conv in eval
}
CASES = {**TRAIN, **EVAL}
ODD_BOTTLENECK = ("r50-odd", "r50-odd-eval")
FALLBACK = ("r50-fallback", "r50-fallback-eval")


def _half(n):
    """output size of a stride-2 window that covers the input with symmetric padding (7/2/3, 3/2/1, 1/2/0)"""
    return (n - 1) // 2 + 1


def stage_maps(H, W):
    """[(h, w)] of layer1 .. layer4 for an H x W image: stem and pool halve once each, layer2 - 4 once each"""
    h, w = _half(_half(H)), _half(_half(W))
    out = [(h, w)]
    for _ in range(3):
        h, w = _half(h), _half(w)
        out.append((h, w))
    return out


def tap_shapes(cfg):
    """the (B, h, w, C) shape of every residual block's output, in network order"""
    from oracle import restatement as R
    kind, nblocks = R.RESNET_SPECS[cfg["version"]]
    exp = 4 if kind == "bottleneck" else 1
    return [(cfg["B"], h, w, planes * exp)
            for (h, w), planes, nb in zip(stage_maps(cfg["H"], cfg["W"]), (64, 128, 256, 512), nblocks) for _ in range(nb)]


def layer4_samples(cfg):
    h, w = stage_maps(cfg["H"], cfg["W"])[3]
    return cfg["B"] * h * w


def limits(cfg):
    """A: {'block': (max-rel, L2, per image), 'block0': ...}"""
    return FP32 if cfg["dtype"] == F32 else SMALL


def buffer_limits(cfg):
    """C: (batch mean, variance per channel, variance offset of the layer)"""
    return BUFFER_MEAN, BUFFER_VAR["small"], VAR_OFFSET["small"]


def pool_limit(cfg):
    """D: POOL_MAX for bf16 taps; fp32 taps: an fp32 sum of h * w non-negative values in any order, and the division"""
    h, w = stage_maps(cfg["H"], cfg["W"])[3]
    return h * w * 2.0 ** -24 if cfg["dtype"] == F32 else POOL_MAX


def dtype_name(cfg):
    return "bf16" if cfg["dtype"] == BF16 else "f32"
