"""Tensor-level wrappers over the C ABI (torch supplies device memory and streams only).

Every function checks shapes/dtypes on the host before a kernel is launched and
raises ``ShowTellHipError`` on failure.  All tensors must live on a HIP device.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import (BnActDesc, ConvB2bDesc, ConvC3c1Desc, Conv1x1KfuseDesc, Conv1x1WregDesc, Conv3x3ImgDesc, ConvDesc, StemConvPoolDesc,
                   check, dtype_code, lib)
from ._lib import ptr as _p, stream as _stream  # noqa: F401  (the names this module has always used; tools import them)

_DT = _lib._DTYPE_CODES


def dt_code(t):
    return dtype_code(t.dtype)


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.ShowTellHipError("tensor is not on the GPU (the HIP path has no CPU fallback)")
        if t is not None and not t.is_contiguous():
            raise _lib.ShowTellHipError("tensor must be contiguous")


def _set_bn(d, prefix, bn, count=False, replicas=None):
    """Describe the batch norm `bn` = dict(stats, gamma, beta[, count, eps, replicas]) in the fields `prefix`_stats / _gamma /
    _beta of descriptor `d`; count: also `prefix`_count / _eps; replicas: the name of d's replica-count field for these
    statistics, where it has one.  bn None: the fields stay NULL / 0."""
    if bn is None:
        return
    _dev(bn["stats"], bn["gamma"], bn["beta"])
    for f in ("stats", "gamma", "beta"):
        setattr(d, f"{prefix}_{f}", bn[f].data_ptr())
    if count:
        setattr(d, prefix + "_count", float(bn["count"]))
        setattr(d, prefix + "_eps", float(bn.get("eps", 1e-5)))
    if replicas:
        setattr(d, replicas, int(bn.get("replicas", 0)))


def conv_nhwc(x, w, KH, KW, stride, pad, out_dtype=None, bias=None, scale=None, shift=None,
              residual=None, stats=None, relu=False, out=None, accumulate=False, k_order=0, stats_replicas=0,
              in_bn=None):
    """x: (B,Hin,Win,Cin) NHWC; w: (N, KH*KW*Cin) K-contiguous.  Returns (B,Ho,Wo,N).
    stats_replicas = R > 1: stats is (R, 2N), pixel tile t adds into replica t % R.
    in_bn = dict(stats, gamma, beta, count[, eps]): x is a producer's raw output, the conv reads relu(batchnorm(x))."""
    _dev(x, w, bias, scale, shift, residual, stats, out)
    B, Hin, Win, Cin = x.shape
    N = w.shape[0]
    assert w.shape[1] == KH * KW * Cin, (w.shape, KH, KW, Cin)
    Ho = (Hin + 2 * pad - KH) // stride + 1
    Wo = (Win + 2 * pad - KW) // stride + 1
    out_dtype = out_dtype or x.dtype
    if out is None:
        out = torch.empty(B, Ho, Wo, N, device=x.device, dtype=out_dtype)
    assert out.shape == (B, Ho, Wo, N) and out.dtype == out_dtype
    d = ConvDesc(x=_p(x), w=_p(w), y=_p(out), bias=_p(bias), scale=_p(scale), shift=_p(shift), residual=_p(residual), stats=_p(stats),
                 dtype=dtype_code(x.dtype), out_dtype=_DT[out_dtype], B=B, Hin=Hin, Win=Win, Cin=Cin, Ho=Ho, Wo=Wo, N=N,
                 KH=KH, KW=KW, stride=stride, pad=pad, ldx=Cin, ldw=w.shape[1], ldy=N, relu=int(relu), accumulate=int(accumulate),
                 k_order=int(k_order), stats_replicas=int(stats_replicas))
    _set_bn(d, "in", in_bn, count=True)
    check(lib().st_conv(C.byref(d), _stream()), "st_conv")
    return out


def _s2d_images(images, dtype):
    """(B,3,H,W) fp32 -> the stem's space-to-depth input (B, H/2+3, W/2+3, 16) (st_nchw_to_s2d16)."""
    B, Cc, H, W = images.shape
    assert Cc == 3 and images.dtype == torch.float32
    xs = torch.empty(B, H // 2 + 3, W // 2 + 3, 16, device=images.device, dtype=dtype)
    check(lib().st_nchw_to_s2d16(_p(images), _p(xs), _DT[dtype], B, H, W, _stream()), "st_nchw_to_s2d16")
    return xs


def stem_weight_s2d(w_packed, cpad, dtype):
    """The (64, 7*7*cpad) k_order-0 stem filters as the (64, 256) operand of the space-to-depth route (st_stem_weight_s2d)."""
    _dev(w_packed)
    ws = torch.empty(64, 256, device=w_packed.device, dtype=dtype)
    check(lib().st_stem_weight_s2d(_p(w_packed), _p(ws), _DT[dtype], cpad, _stream()), "st_stem_weight_s2d")
    return ws


def stem_weight_frag_from_s2d(ws):
    """stem_weight_s2d's bf16 result in st_stem_conv_pool's fragment order (st_stem_weight_frag)."""
    _dev(ws)
    wf = torch.empty(64 * 256, device=ws.device, dtype=torch.bfloat16)
    check(lib().st_stem_weight_frag(_p(ws), _p(wf), _stream()), "st_stem_weight_frag")
    return wf


def stem_weight_frag(w_packed, cpad):
    """The same operand in one launch from the bf16 (64, 7*7*cpad) filters (st_stem_weight_frag_packed, as st_resnet_forward packs)."""
    _dev(w_packed)
    wf = torch.empty(64 * 256, device=w_packed.device, dtype=torch.bfloat16)
    check(lib().st_stem_weight_frag_packed(_p(w_packed), int(cpad), _p(wf), _stream()), "st_stem_weight_frag_packed")
    return wf


def stem_conv_s2d(images, w_packed, cpad, dtype, stats=None, scale=None, shift=None, relu=False):
    """torchvision stem (7x7 s2 p3 over RGB, cnn.py:46) through the space-to-depth route: images (B,3,H,W) fp32 with
    even H, W; w_packed the usual (64, 7*7*cpad) k_order-0 weights.  Returns (B,H/2,W/2,64)."""
    _dev(images, w_packed, stats, scale, shift)
    B, _, H, W = images.shape
    xs = _s2d_images(images, dtype)
    ws = stem_weight_s2d(w_packed, cpad, dtype)
    out = torch.empty(B, H // 2, W // 2, 64, device=images.device, dtype=dtype)
    d = ConvDesc(x=_p(xs), w=_p(ws), y=_p(out), scale=_p(scale), shift=_p(shift), stats=_p(stats), dtype=_DT[dtype], out_dtype=_DT[dtype],
                 B=B, Hin=H // 2 + 3, Win=W // 2 + 3, Cin=64, Ho=H // 2, Wo=W // 2, N=64, KH=4, KW=1, stride=1, pad=0,
                 ldx=16, ldw=256, ldy=64, relu=int(relu), Cin_logical=36)
    check(lib().st_conv(C.byref(d), _stream()), "st_conv(s2d stem)")
    return out, xs, ws


def stem_conv_pool(images, w_packed, cpad, stats=None, stats_replicas=0, gamma=None, scale=None, shift=None):
    """The bf16 stem in one kernel (st_stem_conv_pool): conv 7x7/2 + statistics + maxpool 3x3/2.  images (B,3,H,W) fp32, even H, W;
    w_packed the usual (64, 7*7*cpad) bf16 k_order-0 weights.  Train (gamma, stats): the pooled RAW output (max / min by sign(gamma));
    eval (scale, shift): maxpool(relu(conv * scale + shift)).  Returns (B, PH, PW, 64) bf16."""
    _dev(images, w_packed, stats, gamma, scale, shift)
    B, _, H, W = images.shape
    xs = _s2d_images(images, torch.bfloat16)
    wf = stem_weight_frag(w_packed, cpad)
    PH, PW = (H // 2 - 1) // 2 + 1, (W // 2 - 1) // 2 + 1
    out = torch.empty(B, PH, PW, 64, device=images.device, dtype=torch.bfloat16)
    d = StemConvPoolDesc(x_s2d=_p(xs), w_frag=_p(wf), y=_p(out), stats=_p(stats), stats_replicas=int(stats_replicas), gamma=_p(gamma),
                         scale=_p(scale), shift=_p(shift), B=B, H=H, W=W)
    check(lib().st_stem_conv_pool(C.byref(d), _stream()), "st_stem_conv_pool")
    return out


def _gemm_desc(a, w, out, K, lda, ldw, **fields):
    return ConvDesc(x=_p(a), w=_p(w), y=_p(out), dtype=dtype_code(a.dtype), out_dtype=_DT[out.dtype], B=a.shape[0], Hin=1, Win=1, Cin=K,
                    Ho=1, Wo=1, N=w.shape[0], KH=1, KW=1, stride=1, pad=0, ldx=lda, ldw=ldw, ldy=out.stride(0), **fields)


def gemm_nt(a, w, out_dtype=None, bias=None, out=None, accumulate=False, stats=None, relu=False,
            lda=None, ldw=None, K=None, split_k=0):
    """y[M,N] = a[M,K] @ w[N,K]^T (+bias).  a, w may carry padded leading dimensions."""
    _dev(a, w, bias, out, stats)
    if out is None:
        out = torch.empty(a.shape[0], w.shape[0], device=a.device, dtype=out_dtype or a.dtype)
    d = _gemm_desc(a, w, out, K or a.shape[1], lda or a.stride(0), ldw or w.stride(0), bias=_p(bias), stats=_p(stats),
                   relu=int(relu), accumulate=int(accumulate), split_k=int(split_k))
    check(lib().st_conv(C.byref(d), _stream()), "st_conv(gemm)")
    return out


def gemm_nt_batch(As, Ws, outs, accumulate=False):
    """Several y_i[M,N] (+)= a_i[M,K] @ w_i[N,K]^T of identical shape as ONE launch (st_conv_batch)."""
    n = len(As)
    arr = (ConvDesc * n)()
    for i, (a, w, o) in enumerate(zip(As, Ws, outs)):
        _dev(a, w, o)
        arr[i] = _gemm_desc(a, w, o, a.shape[1], a.stride(0), w.stride(0), accumulate=int(accumulate))
    check(lib().st_conv_batch(arr, n, _stream()), "st_conv_batch")
    return outs


def bn_act(x, gamma, beta, stats=None, running=None, count=1.0, eps=1e-5, relu=True, res=None,
           res_bn=None, out=None, stats_replicas=0):
    """x: (..., C) channels-last.  res_bn = dict(gamma, beta, stats | running=(mean,var)) or None."""
    _dev(x, gamma, beta, stats, res, out)
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    if out is None:
        out = torch.empty_like(x)
    rm, rv = running if running is not None else (None, None)
    rb = res_bn or {}
    rrm, rrv = rb.get("running", (None, None))
    d = BnActDesc(x=_p(x), y=_p(out), res=_p(res), stats=_p(stats), gamma=_p(gamma), beta=_p(beta), running_mean=_p(rm), running_var=_p(rv),
                  res_stats=_p(rb.get("stats")), res_gamma=_p(rb.get("gamma")), res_beta=_p(rb.get("beta")),
                  res_running_mean=_p(rrm), res_running_var=_p(rrv), res_bn=int(res_bn is not None), dtype=dtype_code(x.dtype),
                  rows=rows, C=Cc, count=float(count), eps=float(eps), relu=int(relu),
                  stats_replicas=int(stats_replicas), res_stats_replicas=int(rb.get("stats_replicas", 0)))
    check(lib().st_bn_act(C.byref(d), _stream()), "st_bn_act")
    return out


def bn_update_running(stats, running_mean, running_var, count, momentum):
    _dev(stats, running_mean, running_var)
    check(lib().st_bn_update_running(_p(stats), _p(running_mean), _p(running_var), running_mean.numel(),
                                     float(count), float(momentum), _stream()), "st_bn_update_running")


def nchw_to_nhwc(x, dtype, cpad):
    _dev(x)
    assert x.dtype == torch.float32
    B, Cc, H, W = x.shape
    y = torch.empty(B, H, W, cpad, device=x.device, dtype=dtype)
    check(lib().st_nchw_to_nhwc(_p(x), _p(y), _DT[dtype], B, Cc, H, W, cpad, _stream()), "st_nchw_to_nhwc")
    return y


def nhwc_to_ncp_f32(x):
    _dev(x)
    B, H, W, Cc = x.shape
    y = torch.empty(B, Cc, H * W, device=x.device, dtype=torch.float32)
    check(lib().st_nhwc_to_ncp_f32(_p(x), _p(y), dtype_code(x.dtype), B, H * W, Cc, _stream()), "st_nhwc_to_ncp_f32")
    return y


def maxpool3x3s2(x):
    _dev(x)
    B, H, W, Cc = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty(B, Ho, Wo, Cc, device=x.device, dtype=x.dtype)
    check(lib().st_maxpool3x3s2(_p(x), _p(y), dtype_code(x.dtype), B, H, W, Cc, _stream()), "st_maxpool3x3s2")
    return y


def maxpool3x3s2_bn(x, gamma, beta, stats=None, running=None, count=1.0, eps=1e-5):
    """maxpool3x3s2(relu(batchnorm(x))) in one pass (the ResNet stem tail)."""
    _dev(x, gamma, beta, stats)
    B, H, W, Cc = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty(B, Ho, Wo, Cc, device=x.device, dtype=x.dtype)
    rm, rv = running if running is not None else (None, None)
    check(lib().st_maxpool3x3s2_bn(_p(x), _p(y), dtype_code(x.dtype), B, H, W, Cc, _p(stats), _p(gamma), _p(beta), _p(rm), _p(rv),
                                   float(count), float(eps), _stream()), "st_maxpool3x3s2_bn")
    return y


def global_avgpool(x, out_dtype=None):
    _dev(x)
    B, H, W, Cc = x.shape
    out_dtype = out_dtype or x.dtype
    y = torch.empty(B, Cc, device=x.device, dtype=out_dtype)
    check(lib().st_global_avgpool(_p(x), _p(y), dtype_code(x.dtype), _DT[out_dtype], B, H * W, Cc, _stream()), "st_global_avgpool")
    return y


def cast(x, dtype, out=None):
    _dev(x, out)
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=dtype)
    check(lib().st_cast(_p(x), _p(out), dtype_code(x.dtype), _DT[dtype], x.numel(), _stream()), "st_cast")
    return out


def transpose(x, ldy=None, out=None, colsum=None):
    """x: (rows, cols) -> (cols, ldy) with ldy >= rows, zero padded; colsum (cols,) fp32 += column sums of x."""
    _dev(x, out, colsum)
    rows, cols = x.shape
    ldy = ldy or rows
    if out is None:
        out = torch.empty(cols, ldy, device=x.device, dtype=x.dtype)
    check(lib().st_transpose_colsum(_p(x), _p(out), _p(colsum), dtype_code(x.dtype), rows, cols, x.stride(0), ldy, _stream()),
          "st_transpose_colsum")
    return out


def pack_conv_weight_frag(w, ntw):
    """(Cout,Cin,KH,KW) fp32 torch layout -> fragment-major bf16 (st_pack_conv_weight_frag) for the image-resident kernels."""
    _dev(w)
    Cout, Cin, KH, KW = w.shape
    out = torch.empty(Cout * KH * KW * Cin, device=w.device, dtype=torch.bfloat16)
    check(lib().st_pack_conv_weight_frag(_p(w), _p(out), Cout, Cin, KH, KW, int(ntw), _stream()), "st_pack_conv_weight_frag")
    return out


def conv3x3_img_supported(H, W, C, N):
    return int(lib().st_conv3x3_img_supported(H, W, C, N))


def _conv3x3(entry, name, out_hw, x, w_frag, N, stats, stats_replicas, scale, shift, relu, in_bn, out):
    """conv3x3_img and conv3x3_s2: one descriptor type, `entry` and the output's (Ho, Wo) differ."""
    _dev(x, w_frag, stats, scale, shift, out)
    B, H, W, Cc = x.shape
    if x.dtype != torch.bfloat16:
        raise _lib.ShowTellHipError(f"{name} is a bf16 kernel")
    if out is None:
        out = torch.empty(B, *out_hw(H, W), N, device=x.device, dtype=torch.bfloat16)
    d = Conv3x3ImgDesc(x=_p(x), w_frag=_p(w_frag), y=_p(out), stats=_p(stats), stats_replicas=int(stats_replicas), scale=_p(scale),
                       shift=_p(shift), relu=int(relu), B=B, H=H, W=W, C=Cc, N=N)
    _set_bn(d, "in", in_bn, count=True, replicas="in_stats_replicas")
    check(entry(C.byref(d), _stream()), "st_" + name)
    return out


def conv3x3_img(x, w_frag, N, stats=None, stats_replicas=0, scale=None, shift=None, relu=False, in_bn=None, out=None):
    """Image-resident 3x3 s1 p1 conv (st_conv3x3_img): x (B,H,W,C) bf16 NHWC, w_frag from pack_conv_weight_frag."""
    return _conv3x3(lib().st_conv3x3_img, "conv3x3_img", lambda H, W: (H, W),
                    x, w_frag, N, stats, stats_replicas, scale, shift, relu, in_bn, out)


def conv3x3_s2_supported(Cin, N):
    return int(lib().st_conv3x3_s2_supported(Cin, N))


def conv3x3_s2(x, w_frag, N, stats=None, stats_replicas=0, scale=None, shift=None, relu=False, in_bn=None, out=None):
    """K-streaming 3x3 stride-2 pad-1 conv (st_conv3x3_s2): x (B,H,W,C) bf16 NHWC, w_frag = pack_conv_weight_frag(w, conv3x3_s2_supported(C, N))."""
    return _conv3x3(lib().st_conv3x3_s2, "conv3x3_s2", lambda H, W: ((H - 1) // 2 + 1, (W - 1) // 2 + 1),
                    x, w_frag, N, stats, stats_replicas, scale, shift, relu, in_bn, out)


def _conv1x1(entry, name, x, w_frag, N, stride, stats, stats_replicas, scale, shift, relu, out, residual=None, in_bn=None,
             stats_only=False):
    """conv1x1_wreg, conv1x1_astat and conv1x1_kstream: one descriptor type, `entry` and the optional arguments each takes differ.
    stats_only: y == NULL -- only the [sum | sumsq] statistics of the output are produced (returns None)."""
    _dev(x, w_frag, stats, scale, shift, residual, out)
    B, H, W, Cc = x.shape
    if x.dtype != torch.bfloat16:
        raise _lib.ShowTellHipError(f"{name} is a bf16 kernel")
    if out is None and not stats_only:
        out = torch.empty(B, (H - 1) // stride + 1, (W - 1) // stride + 1, N, device=x.device, dtype=torch.bfloat16)
    d = Conv1x1WregDesc(x=_p(x), w_frag=_p(w_frag), y=_p(out), residual=_p(residual), stats=_p(stats), stats_replicas=int(stats_replicas),
                        scale=_p(scale), shift=_p(shift), relu=int(relu), B=B, Hin=H, Win=W, C=Cc, N=N, stride=int(stride))
    _set_bn(d, "in", in_bn, count=True, replicas="in_stats_replicas")
    check(entry(C.byref(d), _stream()), "st_" + name)
    return out


def conv1x1_wreg_supported(Cin, N):
    return int(lib().st_conv1x1_wreg_supported(Cin, N))


def conv1x1_wreg(x, w_frag, N, stride=1, stats=None, stats_replicas=0, scale=None, shift=None, relu=False, residual=None, in_bn=None, out=None,
                 stats_only=False):
    """Register-resident-filter 1x1 conv (st_conv1x1_wreg): x (B,H,W,C) bf16 NHWC, w_frag from pack_conv_weight_frag(w (N,C,1,1)).
    stats_only: y == NULL -- only the [sum | sumsq] statistics of the output are produced (returns None)."""
    return _conv1x1(lib().st_conv1x1_wreg, "conv1x1_wreg", x, w_frag, N, stride, stats, stats_replicas, scale, shift, relu, out,
                    residual, in_bn, stats_only)


def conv1x1_kfuse_supported(Cin, N):
    return int(lib().st_conv1x1_kfuse_supported(Cin, N))


def conv1x1_kfuse(raw, identity, w_frag, bn, N=256, id_bn=None, stats=None, stats_replicas=0, x_out=None, out=None, eight_waves=False):
    """st_conv1x1_kfuse: x = relu(bn(raw) + identity) (written to x_out; identity normalised with id_bn first when given),
    y = conv1x1(x) (C -> N).  bn / id_bn = dict(stats, gamma, beta[, count, eps, replicas]).  Returns (x_out, y)."""
    _dev(raw, identity, w_frag, stats, x_out, out)
    rows = raw.numel() // raw.shape[-1]
    if x_out is None:
        x_out = torch.empty_like(raw)
    if out is None:
        out = torch.empty(*raw.shape[:-1], N, device=raw.device, dtype=torch.bfloat16)
    d = Conv1x1KfuseDesc(raw=_p(raw), identity=_p(identity), x_out=_p(x_out), w_frag=_p(w_frag), y=_p(out), stats=_p(stats),
                         stats_replicas=int(stats_replicas), rows=rows, C=raw.shape[-1], N=N)
    _set_bn(d, "f", bn, count=True, replicas="f_stats_replicas")
    _set_bn(d, "id", id_bn, replicas="id_stats_replicas")
    if eight_waves:
        check(lib().st_conv1x1_kfuse8(C.byref(d), _stream()), "st_conv1x1_kfuse8")
    else:
        check(lib().st_conv1x1_kfuse(C.byref(d), _stream()), "st_conv1x1_kfuse")
    return x_out, out


def conv_b2b(raw2, w3_frag, identity, w1_frag, N, bn2, bn3, count, id_bn=None, eps=1e-5, stats=None, stats_replicas=0, x_out=None, out=None):
    """st_conv_b2b: x = relu(bn3(conv3(relu(bn2(raw2)))) + identity) (written to x_out), y = conv1(x) (N == 0: no conv1, y is None).
    bn2 / bn3 / id_bn = dict(stats, gamma, beta[, replicas]).  Returns (x_out, y)."""
    _dev(raw2, w3_frag, identity, w1_frag, stats, x_out, out)
    rows = raw2.numel() // raw2.shape[-1]
    if x_out is None:
        x_out = torch.empty_like(identity)
    if out is None and N > 0:
        out = torch.empty(*raw2.shape[:-1], N, device=raw2.device, dtype=torch.bfloat16)
    d = ConvB2bDesc(raw2=_p(raw2), w3_frag=_p(w3_frag), identity=_p(identity), x_out=_p(x_out), w1_frag=_p(w1_frag), y=_p(out),
                    stats=_p(stats), stats_replicas=int(stats_replicas), count=float(count), eps=float(eps),
                    rows=rows, C1=raw2.shape[-1], C2=identity.shape[-1], N=N)
    for prefix, bn in (("bn2", bn2), ("bn3", bn3), ("id", id_bn)):
        _set_bn(d, prefix, bn, replicas=prefix + "_replicas")
    check(lib().st_conv_b2b(C.byref(d), _stream()), "st_conv_b2b")
    return x_out, out


def conv_c3c1(x2, w3_frag, identity, w1_frag, bn2=None, bn3=None, count=None, eps=1e-5, stats=None, stats_replicas=0,
              scale3=None, shift3=None, scale1=None, shift1=None, relu1=True, x_out=None, out=None, id_bn=None):
    """st_conv_c3c1: x = relu(bn3(conv3(a2)) + identity) (-> x_out), y = conv1_next(x) for the 14 x 14 Bottlenecks (256 -> 1024 -> 256)
    and the 28 x 28 ones (128 -> 512 -> 128).
    train: bn3 = dict(stats, gamma, beta[, replicas]) (+ bn2 for a raw x2), count; eval: scale3 / shift3 / scale1 / shift1.  Returns (x_out, y)."""
    _dev(x2, w3_frag, identity, w1_frag, stats, x_out, out, scale3, shift3, scale1, shift1)
    rows = x2.numel() // x2.shape[-1]
    if x_out is None:
        x_out = torch.empty_like(identity)
    if out is None:
        out = torch.empty(*x2.shape[:-1], x2.shape[-1], device=x2.device, dtype=torch.bfloat16)
    d = ConvC3c1Desc(x2=_p(x2), w3_frag=_p(w3_frag), identity=_p(identity), x_out=_p(x_out), w1_frag=_p(w1_frag), y=_p(out),
                     stats=_p(stats), stats_replicas=int(stats_replicas), count=float(count or 0.0), eps=float(eps),
                     scale3=_p(scale3), shift3=_p(shift3), scale1=_p(scale1), shift1=_p(shift1), relu1=int(relu1),
                     rows=rows, C1=x2.shape[-1], C2=identity.shape[-1], N=out.shape[-1])
    for prefix, bn in (("bn2", bn2), ("bn3", bn3), ("id", id_bn)):
        _set_bn(d, prefix, bn, replicas=prefix + "_replicas")
    check(lib().st_conv_c3c1(C.byref(d), _stream()), "st_conv_c3c1")
    return x_out, out


def conv1x1_astat_supported(Cin, N):
    return int(lib().st_conv1x1_astat_supported(Cin, N))


def conv1x1_astat(x, w_frag, N, stride=1, stats=None, stats_replicas=0, scale=None, shift=None, relu=False, in_bn=None, out=None, residual=None,
                  stats_only=False):
    """Activation-stationary 1x1 conv (st_conv1x1_astat): stride 1 with (C, N) in {(256, 1024), (512, 2048)}, stride 2 with (256, 512) /
    (512, 1024); w_frag = pack_conv_weight_frag(w, conv1x1_astat_supported(C, N))."""
    return _conv1x1(lib().st_conv1x1_astat, "conv1x1_astat", x, w_frag, N, stride, stats, stats_replicas, scale, shift, relu, out,
                    residual, in_bn, stats_only)


def conv1x1_kstream_supported(Cin, N):
    return int(lib().st_conv1x1_kstream_supported(Cin, N))


def conv1x1_kstream(x, w_frag, N, stride=1, stats=None, stats_replicas=0, scale=None, shift=None, relu=False, out=None):
    """Long-K 1x1 conv (st_conv1x1_kstream): x (B,H,W,C) bf16 NHWC with C in {1024, 2048}, w_frag = pack_conv_weight_frag(w, 4)."""
    return _conv1x1(lib().st_conv1x1_kstream, "conv1x1_kstream", x, w_frag, N, stride, stats, stats_replicas, scale, shift, relu, out)


def pack_conv_weight(w, dtype, cpad=None, k_order=0):
    """(Cout,Cin,KH,KW) fp32 torch layout -> (Cout, KH*KW*Cpad) K-contiguous (k_order: see st_conv_desc)."""
    _dev(w)
    Cout, Cin, KH, KW = w.shape
    cpad = cpad or Cin
    out = torch.empty(Cout, KH * KW * cpad, device=w.device, dtype=dtype)
    check(lib().st_pack_conv_weight(_p(w), _p(out), _DT[dtype], Cout, Cin, KH, KW, cpad, int(k_order), _stream()), "st_pack_conv_weight")
    return out
