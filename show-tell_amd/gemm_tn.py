"""Token-contraction GEMM (csrc/gemm_tn.hip): ``c (+)= a^T b`` for bf16 ``a [K, M]`` and ``b [K, N]`` as they lie.

The decoder backward calls the C entry point itself (st_rnn_backward); this wrapper serves tests and tools.
"""
import ctypes as C

import torch

from ._lib import ST_BF16, ShowTellHipError, check, lib, ptr, stream

c_p, c_i = C.c_void_p, C.c_int


class GemmTnDesc(C.Structure):
    """Mirror of st_gemm_tn_desc (layout checked by tests/test_tn_tile_map.py)."""
    _fields_ = [("a", c_p), ("b", c_p), ("c", c_p), ("b_row", c_p), ("b_live", c_p), ("colsum0", c_p), ("colsum1", c_p),
                ("dtype", c_i), ("M", c_i), ("N", c_i), ("K", c_i), ("lda", c_i), ("ldb", c_i), ("ldc", c_i), ("accumulate", c_i)]


def desc(a, b, c, M, N, K=None, b_row=None, b_live=None, colsum0=None, colsum1=None, accumulate=False):
    """One problem.  a: [K, lda] bf16, b: [rows, ldb] bf16, c: [M, ldc] fp32, all 2-d with unit column stride; the
    leading dimensions are the tensors' row strides, so views with pad columns pass as they are."""
    for t in (a, b, c):
        if not t.is_cuda or t.dim() != 2 or t.stride(1) != 1:
            raise ShowTellHipError("gemm_tn: operands must be 2-d device tensors with unit column stride")
    if a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16 or c.dtype != torch.float32:
        raise ShowTellHipError("gemm_tn: a and b are bfloat16, c is float32")
    return GemmTnDesc(a=ptr(a), b=ptr(b), c=ptr(c), b_row=ptr(b_row), b_live=ptr(b_live), colsum0=ptr(colsum0), colsum1=ptr(colsum1),
                      dtype=ST_BF16, M=M, N=N, K=a.shape[0] if K is None else K, lda=a.stride(0), ldb=b.stride(0), ldc=c.stride(0),
                      accumulate=int(bool(accumulate)))


def gemm_tn_batch(descs):
    """Up to 12 problems (GemmTnDesc) of any mix of shapes as one launch on the current stream."""
    arr = (GemmTnDesc * max(len(descs), 1))(*descs)
    check(lib().st_gemm_tn_batch(arr, len(descs), stream()), "st_gemm_tn_batch")
