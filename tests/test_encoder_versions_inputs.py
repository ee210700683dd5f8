"""The inputs and bounds of tests/test_gpu_encoder_versions.py have the power to catch a fault: shown from the float64 oracle
alone.  Nothing here needs a GPU.

"Got" is a CPU emulation of bf16 storage: the float64 oracle block with every convolution output, and the block output, rounded
to bf16 (BatchNorm statistics are taken over the stored values; the running buffers are updated in fp32 with the kernel's
constants).  It is walked as the GPU test walks the kernels -- block k of the oracle starts from the emulation's tap k - 1 --
and judged by the GPU file's own checks and bounds (failures_elementwise: A, failures_running_buffers: C).

clean   ResNet-18 and -34, train B = 5 and eval B = 3: the emulation passes A and C.  This is the statement that the reference
        alone, stored in bf16, stays within the bounds.
faults  each seeded into the emulation of one block (from the clean tap before it); the named check must fail:
          ds-no-bn      layer2.0 adds the downsample convolution without its BatchNorm                                  A
          no-residual   one block, eval mode: the identity is not added                                                 A
          zero-row      the last output row of one image of one stride-2 3 x 3 convolution is zero                       A per image
          b-minus-1     one layer's batch statistics cover B - 1 images                                                  C
          replica       one of four statistics replicas (128-row tiles, round robin) is left out of the sums             C
          biased-var    the biased variance is absorbed: off by 1 / 245 = 4.1e-3 in layer4, in every channel alike     C (offset)
        and two kinds that tests/test_encoder_sizes_inputs.py seeds at other image sizes:
          pad-column    a 3 x 3 convolution reads the column beyond W as the first column of the next row               A
          pool-49       the pooled mean divides by 49, not by h * w                                                     D

`python -m tests.test_encoder_versions_inputs` prints the figures of every case."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import restatement as R
from tests._encoder_walk import KEEP32, MOM32, _bf16, _block_metrics, _blocks, _double, _params, _running, _stem_pool
from tests.test_gpu_encoder_versions import _cfg, buffer_limits, failures_elementwise, failures_running_buffers, limits

EPS = 1e-5
CLEAN = [(18, True), (18, False), (34, True), (34, False)]


def _store(t):
    """one bf16 storage rounding of a float64 tensor"""
    return _bf16(t.float()).double()


class Emulation:
    """The oracle's block (R.block_forward) in float64 with bf16 storage, and the faults.  `fault`: (kind, where) or None; `where`
    is a conv / BatchNorm key prefix."""

    def __init__(self, p, train, fault=None):
        self.p, self.train, self.fault = p, train, fault or (None, None)
        self.absorbed = {}          # bn -> (mean, variance) the running buffers absorb

    def _is(self, kind, where):
        return self.fault == (kind, where)

    def conv(self, x, key, stride, pad):
        if self._is("pad-column", key):
            # the column beyond W is read as the first column of the NEXT row, not as zero: what a flat (row * W + column)
            # index does without a pad column.  The last row's neighbour stays zero.
            assert pad == 1
            x = F.pad(x, (1, 1, 1, 1))
            x[:, :, 1:-2, -1] = x[:, :, 2:-1, 1]
            pad = 0
        o = _store(F.conv2d(x, self.p[key + ".weight"], None, stride, pad))
        if self._is("zero-row", key):
            o[1, :, -1, :] = 0.0
        return o

    def bn(self, c, bn):
        p = self.p
        if not self.train:
            mean, var = p[bn + ".running_mean"], p[bn + ".running_var"]
        else:
            rows = c.permute(0, 2, 3, 1).reshape(-1, c.shape[1])            # NHWC rows, as the kernels tile them
            n = rows.shape[0]
            if self._is("b-minus-1", bn):
                rows = rows[: n - n // c.shape[0]]
                n = rows.shape[0]
            if self._is("replica", bn):
                tile = torch.arange(n) // 128
                rows = rows[tile % 4 != 3]                                  # the count stays n
            mean = rows.sum(0) / n
            var = (rows * rows).sum(0) / n - mean * mean
            self.absorbed[bn] = (mean, var if self._is("biased-var", bn) else var * n / (n - 1))
        sh = (1, -1, 1, 1)
        return (c - mean.view(sh)) / (var.view(sh) + EPS).sqrt() * p[bn + ".weight"].view(sh) + p[bn + ".bias"].view(sh)

    def block(self, x, version, li, bi):
        kind, _ = R.RESNET_SPECS[version]
        q = f"model.{4 + li}.{bi}"
        s = (1 if li == 0 else 2) if bi == 0 else 1
        idt = x
        if kind == "bottleneck":
            o = F.relu(self.bn(self.conv(x, q + ".conv1", 1, 0), q + ".bn1"))
            o = F.relu(self.bn(self.conv(o, q + ".conv2", s, 1), q + ".bn2"))
            o = self.bn(self.conv(o, q + ".conv3", 1, 0), q + ".bn3")
        else:
            o = F.relu(self.bn(self.conv(x, q + ".conv1", s, 1), q + ".bn1"))
            o = self.bn(self.conv(o, q + ".conv2", 1, 1), q + ".bn2")
        if q + ".downsample.0.weight" in self.p:
            idt = self.conv(x, q + ".downsample.0", s, 0)
            if not self._is("ds-no-bn", q):
                idt = self.bn(idt, q + ".downsample.1")
        if self._is("no-residual", q):
            idt = 0.0
        return _store(F.relu(o + idt))

    def stem(self, image):
        o = F.relu(self.bn(self.conv(image, "model.0", 2, 3), "model.1"))
        return F.max_pool2d(o, 3, 2, 1)

    def pool(self, x):
        """the pooled features of the last tap: an fp32 sum over the pixels, divided by their count"""
        n = 49 if self.fault[0] == "pool-49" else x.shape[2] * x.shape[3]
        return (x.float().sum((2, 3)) / n).double()

    def buffers(self, before):
        """`before` after the momentum updates of what was absorbed: fp32, the kernel's constants"""
        out = {k: v.clone() for k, v in before.items()}
        for bn, (mean, var) in self.absorbed.items():
            for key, stat in (("running_mean", mean), ("running_var", var)):
                out[f"{bn}.{key}"] = (KEEP32 * before[f"{bn}.{key}"].double() + MOM32 * stat).float()
            out[bn + ".num_batches_tracked"] = before[bn + ".num_batches_tracked"] + 1
        return out


def _run_dict(cfg, name, blocks, emu, before, oracle_p):
    bns = [bn for *_, bn in R.resnet_conv_list(cfg["version"]) if bn in emu.absorbed] if cfg["train"] else []
    return dict(name=name, cfg=cfg, blocks=blocks, bns=bns, before=before, after=emu.buffers(before), oracle=_running(oracle_p))


def _pool_error(pooled, last):
    """D of the GPU file: the pooled features against the float64 mean of the last tap"""
    pref = last.mean((2, 3))
    return ((pooled - pref).abs().max() / pref.abs().max()).item()


@functools.lru_cache(maxsize=None)
def clean(version, train, H=224, W=224, B=None, seed=None, name=None, keep=None):
    """The clean emulation of a configuration of the GPU file, walked against the oracle: the run the GPU file's checks read,
    the emulation's taps (taps[k]: the input of block k; stored in bf16, which holds them exactly, but for the stem's) and the
    parameters.  By default 224 x 224, B = 5 (train) / 3 (eval); tests/test_encoder_sizes_inputs.py passes its cases' sizes, seeds
    and names, and `keep`: the blocks whose input tap is kept (all by default)."""
    B = B or (5 if train else 3)
    cfg = _cfg(version, B, train, seed=70 + version + train if seed is None else seed, H=H, W=W)
    params = _params(cfg["seed"], version)
    image = _bf16(torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(cfg["seed"]))).double()
    p, before = _double(params), {k: v.clone() for k, v in _running(params).items()}
    emu = Emulation(_double(params), train)
    mets, taps, shapes = [], [], []
    with torch.no_grad():
        xin = _stem_pool(p, image, train)
        got = emu.stem(image)
        for k, li, bi, bname in _blocks(version):
            ref = R.block_forward(p, xin, version, li, bi, train)
            taps.append(None if keep is not None and k not in keep else got if k == 0 else got.bfloat16())
            got = emu.block(got, version, li, bi)
            met = _block_metrics(got, ref, moments=False)
            met.update(k=k, name=bname)
            mets.append(met)
            shapes.append((B, got.shape[2], got.shape[3], got.shape[1]))
            xin = got
        run =_run_dict(cfg, name or f"r{version}-{'train' if train else 'eval'}", mets, emu, before, p)
        run["pool"] = _pool_error(emu.pool(got), got)
        run["tap_shapes"] = shapes
    return dict(run=run, taps=taps, last=got.bfloat16(), params=params, before=before)


def faulted(version, train, k, fault, **case):
    """Block k alone, from the clean tap before it: the oracle against the emulation with `fault`.  case: clean()'s other
    arguments"""
    c = clean(version, train, **case)
    _, li, bi, bname = _blocks(version)[k]
    p = _double(c["params"])
    emu = Emulation(_double(c["params"]), train, fault)
    with torch.no_grad():
        tap = c["taps"][k].double()
        ref = R.block_forward(p, tap, version, li, bi, train)
        got = emu.block(tap, version, li, bi)
    met = _block_metrics(got, ref, moments=False)
    met.update(k=k, name=bname)
    return _run_dict(c["run"]["cfg"], f"{case.get('name') or 'r%d' % version} {bname} {fault[0] if fault else 'clean'}", [met], emu, c["before"], p)


def _figures(run):
    b = max(run["blocks"], key=lambda b: b["img"])
    s = f"{run['name']}: A max-rel {max(x['max'] for x in run['blocks']):.2e}, L2 {max(x['l2'] for x in run['blocks']):.2e}, " \
        f"per image {b['img']:.2e} ({b['name']})"
    if run["cfg"]["train"]:
        _, wm, wv, wo = failures_running_buffers(run)
        s += f"; C batch mean {wm[0]:.2e} ({wm[1]}), variance {wv[0]:.2e} ({wv[1]}), variance offset {wo[0]:.2e} ({wo[1]})"
    return s


@pytest.mark.parametrize("version,train", CLEAN)
def test_the_reference_in_bf16_storage_stays_within_the_bounds(version, train):
    run = clean(version, train)["run"]
    print("MEASURE", _figures(run))
    assert len(run["blocks"]) == sum(R.RESNET_SPECS[version][1])
    assert not failures_elementwise(run)
    if train:
        assert len(run["bns"]) == len(R.resnet_conv_list(version))
        assert not failures_running_buffers(run)[0]


def _block_index(version, name):
    return next(k for k, *_, n in _blocks(version) if n == name)


# A: (version, train, block, fault kind, key the fault sits at)
A_FAULTS = [
    (18, True, "layer2.0", "ds-no-bn", "model.5.0"), (34, False, "layer2.0", "ds-no-bn", "model.5.0"),
    (18, False, "layer1.1", "no-residual", "model.4.1"), (34, False, "layer3.4", "no-residual", "model.6.4"),
    (34, False, "layer4.2", "no-residual", "model.7.2"),
]


@pytest.mark.parametrize("version,train,block,kind,where", A_FAULTS)
def test_a_structural_fault_fails_the_elementwise_check(version, train, block, kind, where):
    run = faulted(version, train, _block_index(version, block), (kind, where))
    print("MEASURE", _figures(run))
    assert failures_elementwise(run)


@pytest.mark.parametrize("version,train,block", [(18, True, "layer2.0"), (34, True, "layer3.0"), (34, False, "layer4.0"),
                                                 (18, False, "layer4.0")])
def test_a_zeroed_row_of_one_image_fails_the_per_image_check(version, train, block):
    """The last output row of image 1 of the block's stride-2 3 x 3 convolution is zero.  The per-image figure catches it; so
    does the plain max-rel, since the error is as large as the activations themselves.  L2 is reported with them: the row is one
    of 7 - 28 in one of 3 - 5 images, and L2 alone sees it only where it is asserted below."""
    q = "model.%d.0" % (3 + int(block[5]))
    run = faulted(version, train, _block_index(version, block), ("zero-row", q + ".conv1"))
    b = run["blocks"][0]
    print("MEASURE", _figures(run), "image", b["img_at"], "at", b["at"])
    lim_mx, lim_l2, lim_img = limits(run["cfg"])["block"]
    assert b["img"] > lim_img and b["img_at"] == 1 and b["at"][0] == 1
    assert b["max"] > lim_mx
    assert b["l2"] > lim_l2


# C: (version, block, fault kind, BatchNorm layer)
C_FAULTS = [
    (18, "layer1.0", "b-minus-1", "model.4.0.bn1"), (34, "layer2.0", "b-minus-1", "model.5.0.downsample.1"),
    (34, "layer4.1", "b-minus-1", "model.7.1.bn2"),
    (18, "layer2.0", "replica", "model.5.0.downsample.1"), (34, "layer1.2", "replica", "model.4.2.bn2"),
    (34, "layer3.0", "replica", "model.6.0.downsample.1"),
    (18, "layer4.1", "biased-var", "model.7.1.bn2"), (34, "layer4.0", "biased-var", "model.7.0.bn1"),
    (34, "layer4.0", "biased-var", "model.7.0.downsample.1"),
]


@pytest.mark.parametrize("version,block,kind,bn", C_FAULTS)
def test_a_statistics_fault_fails_the_running_buffer_check(version, block, kind, bn):
    run = faulted(version, True, _block_index(version, block), (kind, bn))
    bad, wm, wv, wo = failures_running_buffers(run)
    print("MEASURE", _figures(run))
    assert any(line.startswith(bn + ":") for line in bad), (bn, bad)
    if kind == "biased-var":
        # layer4: 5 x 7 x 7 = 245 samples, every channel's variance is short by 1 / 245.  That is BELOW the per-channel bound at
        # B = 5 (storage rounding of 245 values alone comes to 1.7e-3 in the worst channel): the offset over the channels sees it
        _, var_bound, off_bound = buffer_limits(run["cfg"])
        assert 1 / 245 < var_bound and 1 / 245 > 4 * off_bound
        assert wo[1] == bn and abs(wo[0] - 1 / 245) < off_bound
        assert all(line.startswith(bn + ":") for line in bad), bad      # and nothing else moved


if __name__ == "__main__":
    for v, t in CLEAN:
        print(_figures(clean(v, t)["run"]))
    for v, t, block, kind, where in A_FAULTS:
        print(_figures(faulted(v, t, _block_index(v, block), (kind, where))))
    for v, block, kind, bn in C_FAULTS:
        print(_figures(faulted(v, True, _block_index(v, block), (kind, bn))))
