"""st_gemm_tn_batch (csrc/gemm_tn.hip): c (+)= a^T b for bf16 a [K, lda], b [K, ldb] read as they lie, called directly on the
smallest shapes at which it can go wrong.

  K in {1, 31, 32, 33, 135}          below, at and above one LDS image (32 rows) and the 64-row step, two steps plus a tail
  M in {48, 120, 160}, N in {16, 40}  no multiples of the 128-wide tile; 160 spans two row blocks (H = 40 gate widths, in0 = 16)
  M = 1536, N = 512, K = 70           full tiles, 12 x 4 of them
  lda > M, ldb > N                    NaN in the pad columns of both operands (V = 50 -> ld 56)
  gathered b                          negative entries, repeated rows, the b_live table
  accumulate on / off                 on a non-zero prior c
  both column-sum outputs
  10 equal problems / a mix of shapes, each in one launch

The reference is the float64 product of the same bf16 operands.  The bound is the fp32 summation bound of any order,
|got - ref| <= (K + 16) * 2^-24 * (|a|^T |b| + |c_prior|) elementwise, and likewise (K + 16) * 2^-24 * (sum_k |a[k][m]| + |prior|)
for the column sums.  Two calls give the same bits.  Bad arguments return an error and launch nothing.
"""
import pytest
import torch

from showtell_amd import ShowTellHipError
from showtell_amd.gemm_tn import desc, gemm_tn_batch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# MEASURED (MI355X), worst |got - ref| / bound over every case of this file:
#   c 0.059 of the bound, column sums 0.059 of the bound (both at K = 1: one rounding of the sum with the prior value)


def _up8(v):
    return (v + 7) // 8 * 8


class Problem:
    """One problem with its operands on the device and the float64 reference on the host."""

    def __init__(self, M, N, K, seed, lda=None, ldb=None, gather=None, accumulate=False, colsums=0):
        gen = torch.Generator().manual_seed(seed)
        lda, ldb = lda or _up8(M), ldb or _up8(N)
        self.M, self.N, self.K, self.accumulate = M, N, K, accumulate
        a = torch.randn(K, lda, generator=gen).bfloat16()
        a[:, M:] = float("nan")
        rows_b = K if gather is None else K + 3
        b = torch.randn(rows_b, ldb, generator=gen).bfloat16()
        b[:, N:] = float("nan")
        bsel = b[:, :N].double()
        self.b_row = self.b_live = None
        if gather is not None:
            idx = torch.randint(0, rows_b, (K,), generator=gen, dtype=torch.int32)
            idx[::3] = idx[0]                                  # repeated rows
            live = torch.ones(K, dtype=torch.int32)
            if gather == "negative":
                idx[1::4] = -1
                dead = idx < 0
            else:                                              # the packed-sequence convention: rows_t == 0 marks the absent rows
                live[1::4] = 0
                idx[1::4] = 0
                dead = live <= 0
                self.b_live = live.cuda()
            self.b_row = idx.cuda()
            bsel = bsel[idx.clamp(min=0).long()]
            bsel[dead] = 0
        c0 = torch.randn(M, N + 3, generator=gen)              # ldc > N: the columns beyond N must stay what they were
        s0 = torch.randn(2, M, generator=gen)
        ad = a[:, :M].double()
        self.ref = ad.t() @ bsel + (c0[:, :N].double() if accumulate else 0)
        self.mag = ad.abs().t() @ bsel.abs() + (c0[:, :N].double().abs() if accumulate else 0)
        self.cs_ref = ad.sum(0) + s0.double()
        self.cs_mag = ad.abs().sum(0) + s0.double().abs()
        self.c0, self.s0 = c0, s0
        self.a, self.b, self.c = a.cuda(), b.cuda(), c0.clone().cuda()
        self.cs = [s0[i].clone().cuda() for i in range(colsums)]

    def desc(self):
        return desc(self.a, self.b, self.c, self.M, self.N, K=self.K, b_row=self.b_row, b_live=self.b_live,
                    colsum0=self.cs[0] if len(self.cs) > 0 else None, colsum1=self.cs[1] if len(self.cs) > 1 else None,
                    accumulate=self.accumulate)

    def reset(self):
        self.c.copy_(self.c0)
        for i, v in enumerate(self.cs):
            v.copy_(self.s0[i])

    def check(self, tag):
        got = self.c.cpu()
        assert torch.equal(got[:, self.N:], self.c0[:, self.N:]), f"{tag}: columns beyond N were written"
        err = (got[:, :self.N].double() - self.ref).abs()
        bound = (self.K + 16) * U * self.mag
        worst = (err / bound.clamp(min=1e-300)).max().item()
        print(f"MEASURE {tag} c: worst |got - ref| / bound {worst:.3f}")
        assert bool((err <= bound).all()), (tag, worst)
        for i, v in enumerate(self.cs):
            e = (v.cpu().double() - self.cs_ref[i]).abs()
            bd = (self.K + 16) * U * self.cs_mag[i]
            w = (e / bd.clamp(min=1e-300)).max().item()
            print(f"MEASURE {tag} colsum{i}: worst |got - ref| / bound {w:.3f}")
            assert bool((e <= bd).all()), (tag, i, w)
        return [got] + [v.cpu() for v in self.cs]


def _launch(problems, tag):
    gemm_tn_batch([p.desc() for p in problems])
    torch.cuda.synchronize()
    first = [p.check(f"{tag}[{i}]") for i, p in enumerate(problems)]
    for p in problems:
        p.reset()
    gemm_tn_batch([p.desc() for p in problems])
    torch.cuda.synchronize()
    for i, p in enumerate(problems):
        again = [p.c.cpu()] + [v.cpu() for v in p.cs]
        assert all(torch.equal(x, y) for x, y in zip(first[i], again)), f"{tag}[{i}]: two calls differ"


@pytest.mark.parametrize("K", [1, 31, 32, 33, 135])
@pytest.mark.parametrize("M", [48, 120, 160])
@pytest.mark.parametrize("N", [16, 40])
def test_tails(N, M, K):
    seed = 1000 * N + 10 * M + K
    _launch([Problem(M, N, K, seed, accumulate=False, colsums=2)], f"M{M} N{N} K{K} store")
    _launch([Problem(M, N, K, seed + 1, accumulate=True, colsums=1)], f"M{M} N{N} K{K} accumulate")


@pytest.mark.parametrize("accumulate", [False, True], ids=["store", "accumulate"])
def test_full_tiles(accumulate):
    _launch([Problem(1536, 512, 70, 7, accumulate=accumulate, colsums=2)], "full tiles")


@pytest.mark.parametrize("K", [1, 33, 135])
def test_pad_columns_hold_nan(K):
    """lda > M and ldb > N with NaN beyond: V = 50 gives ldd = 56"""
    _launch([Problem(50, 40, K, 50 + K, lda=56, ldb=48, accumulate=True, colsums=1)], f"pad K{K}")
    _launch([Problem(120, 16, K, 60 + K, lda=128, ldb=24, accumulate=False, colsums=2)], f"pad wide K{K}")


@pytest.mark.parametrize("gather", ["negative", "live"])
@pytest.mark.parametrize("K", [31, 135])
def test_gathered_rows(K, gather):
    _launch([Problem(120, 40, K, 70 + K, gather=gather, accumulate=True, colsums=1)], f"gather {gather} K{K}")
    _launch([Problem(160, 16, K, 80 + K, ldb=24, gather=gather, accumulate=False)], f"gather {gather} pad K{K}")


def test_ten_equal_problems_in_one_launch():
    _launch([Problem(120, 40, 33, 100 + i, gather="live" if i % 2 else None, accumulate=True, colsums=1 + i % 2) for i in range(10)],
            "ten equal")


def test_mixed_shapes_in_one_launch():
    ps = [Problem(50, 40, 135, 200, lda=56, accumulate=True, colsums=1),
          Problem(160, 16, 33, 201, accumulate=False, colsums=2),
          Problem(1536, 512, 70, 202, accumulate=True),
          Problem(120, 40, 1, 203, gather="negative", accumulate=True, colsums=2),
          Problem(48, 16, 31, 204, gather="live", accumulate=False, colsums=1)]
    _launch(ps, "mixed")


def test_bad_arguments_return_an_error_and_launch_nothing():
    p = Problem(48, 16, 33, 300, accumulate=False, colsums=1)

    def broken(**kw):
        d = p.desc()
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    bad = {"null a": [broken(a=None)], "null c": [broken(c=None)], "lda below M": [broken(lda=40)], "ldb below N": [broken(ldb=8)],
           "ldc below N": [broken(ldc=8)], "lda no multiple of 8": [broken(lda=52)], "ldb no multiple of 8": [broken(ldb=20)],
           "13 problems": [p.desc()] * 13, "no problem": [], "fp32": [broken(dtype=0)]}
    for what, descs in bad.items():
        with pytest.raises(ShowTellHipError):
            gemm_tn_batch(descs)
        torch.cuda.synchronize()
        assert torch.equal(p.c.cpu(), p.c0) and torch.equal(p.cs[0].cpu(), p.s0[0]), f"{what}: something was launched"
