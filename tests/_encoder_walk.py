"""What the block-by-block float64 walks of the encoder share (tests/test_gpu_encoder_bench_shape.py, tests/test_gpu_encoder_versions.py
and, without a GPU, tests/test_encoder_versions_inputs.py): the parameter randomiser, the oracle's stem, the metrics of one block
output and the batch statistics a running buffer absorbed.  A plain module: no test lives here."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import restatement as R
from tests._util import _bf16  # noqa: F401 (imported from here by other test modules)

MOM32 = float(np.float32(0.1))                   # the kernel's momentum and 1 - momentum, in fp32
KEEP32 = float(np.float32(1.0) - np.float32(0.1))
RUNNING = ("running_mean", "running_var", "num_batches_tracked")


def _params(seed, version=101):
    """R.init_encoder_params(version, 512) with test_gpu_encoder._make(damp=False)'s BatchNorm randomisation; conv weights rounded
    to bf16 so that the oracle and the kernels see the same filters"""
    p = R.init_encoder_params(version, 512, seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    for k in p:
        if k.endswith("running_mean"):
            p[k] = torch.randn(p[k].shape, generator=g) * 0.1
        elif k.endswith("running_var"):
            p[k] = torch.rand(p[k].shape, generator=g) + 0.5
        elif ".bn" in k or k.startswith("model.1.") or "downsample.1" in k:
            if k.endswith(".weight"):
                p[k] = torch.rand(p[k].shape, generator=g) * 0.5 + 0.75
            elif k.endswith(".bias"):
                p[k] = torch.randn(p[k].shape, generator=g) * 0.1
        if p[k].dim() == 4:
            p[k] = _bf16(p[k])
    return p


def _double(params):
    """the oracle's own copy of the parameters, float64 (its running buffers move in place)"""
    return {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in params.items()}


def _running(p):
    """the backbone's running buffers of a parameter / state dictionary"""
    return {k: v for k, v in p.items() if k.startswith("model.") and k.endswith(RUNNING)}


def _stem_pool(p, x, train):
    """the oracle's stem + max pool: what block 0 starts from"""
    return F.max_pool2d(F.relu(R._bn2d(p, F.conv2d(x, p["model.0.weight"], None, 2, 3), "model.1", train)), 3, 2, 1)


def _blocks(version):
    """[(k, li, bi, 'layer<li + 1>.<bi>')] of every residual block in network order"""
    out = []
    for li, nb in enumerate(R.RESNET_SPECS[version][1]):
        for bi in range(nb):
            out.append((len(out), li, bi, f"layer{li + 1}.{bi}"))
    return out


def _nchw64(tap):
    """a (B, h, w, C) tap -> (B, C, h, w) float64, exact"""
    out = torch.empty((tap.shape[0], tap.shape[3], tap.shape[1], tap.shape[2]), dtype=torch.float64)
    out.copy_(tap.permute(0, 3, 1, 2))
    return out


def _block_metrics(got, ref, moments):
    """A (and B if `moments`) of one block output; got, ref (B, C, h, w) float64"""
    ra = ref.abs()
    d = got - ref
    l2 = (d.norm() / ref.norm()).item()
    ad = d.abs_()
    mx = (ad.amax() / ra.amax()).item()
    img = ad.flatten(1).amax(1) / ra.flatten(1).amax(1)
    b, c, y, x = np.unravel_index(int(ad.argmax()), ad.shape)
    out = dict(max=mx, l2=l2, img=img.max().item(), img_at=int(img.argmax()), at=(int(b), int(y), int(x), int(c)))
    if moments:
        sr, mr = torch.std_mean(ref, dim=(0, 2, 3))
        sg, mg = torch.std_mean(got, dim=(0, 2, 3))
        em = (mg - mr).abs() / sr
        es = (sg / sr - 1).abs()
        out.update(mean=em.max().item(), mean_ch=int(em.argmax()), std=es.max().item(), std_ch=int(es.argmax()))
    return out


def _absorbed(after, before, keep=KEEP32, mom=MOM32):
    """the batch statistic a momentum update absorbed: (after - keep * before) / mom, float64"""
    return (after.double() - keep * before.double()) / mom


def _batch_stats(buffers, before, bn, keep=KEEP32, mom=MOM32):
    """(mean, unbiased variance) a layer's running buffers absorbed from `before`"""
    return (_absorbed(buffers[bn + ".running_mean"], before[bn + ".running_mean"], keep, mom),
            _absorbed(buffers[bn + ".running_var"], before[bn + ".running_var"], keep, mom))


def _buffer_errors(after, before, oracle, bn):
    """C of one layer: (|batch mean - oracle's| in units of the oracle's std, |unbiased variance / oracle's - 1|), the worst
    channel of each, and |the mean over the channels of variance / oracle's - 1| (storage rounding averages out over the
    channels, a wrong count does not); `after` holds fp32 buffers updated with the kernel's constants, `oracle` float64 ones"""
    mg, vg = _batch_stats(after, before, bn)
    mo, vo = _batch_stats(oracle, before, bn, 0.9, 0.1)
    rv = vg / vo - 1
    return ((mg - mo).abs() / vo.sqrt()).max().item(), rv.abs().max().item(), abs(rv.mean().item())
