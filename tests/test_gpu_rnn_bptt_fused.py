"""The fused BPTT cell (csrc/rnn_kernels.hip: rnn_bwd_cell_kernel, one launch per reversed diagonal, pull form) against a
float64 oracle (oracle/restatement.py; on bf16-representable weights for the bf16 kernels), against itself (no atomics on the
recurrence: two calls give the same bits) and against the two-launch push route it replaces (ST_BPTT_FUSED=0).

Cases: the smallest shapes at which the cell can go wrong.
  one_cell     L = 1, T = 2, B = 1: no input pair anywhere, no recurrent pair at the last step
  ragged       L = 3, B = 37, packed batch sizes 37, 37, 33, 17, 16, 3: the recurrent pair has fewer rows than the cell, the drop
               crosses a 16-row and a 32-row tile boundary, rows that end mid-sequence get their dy and nothing more
  narrow       E = 16, H = 40, L = 2: in0 != H (the whole-sequence dx0 GEMM on the non-batched W_ih_0 transpose), H no multiple
               of 16, K = 3H = 120 (GRU) no multiple of the K step
  wide         H = 512, L = 2, B = 33, T = 3: full tiles and the row tail of the routed block shape

Bounds.  bf16: GRAD_L2 / GRAD_MAX / ROW_L2 of tests/test_gpu_decoder_bench_shape.py (bf16 storage rounding, 2^-9 per stored
value; both routes consume identical bf16 operands and differ in fp32 summation order only).  fp32: 2e-4 of the tensor's scale,
the bound tests/test_gpu_decoder.py holds the gradients to against gru_small.npz.
The worst errors measured on the MI355X are written below the bounds.
"""
import functools

import pytest
import torch

from oracle import restatement as R
from tests.test_gpu_decoder_bench_shape import (GRAD_L2, GRAD_MAX, ROW_L2, _bf16, _bf16_params, _captions, _decoder, _rel_l2,
                                                _rel_max, _row_l2)

pytestmark = pytest.mark.gpu

FP32_REL = 2e-4     # max |got - ref| / max |ref|, tests/test_gpu_decoder.py

# MEASURED (MI355X), worst over the 16 cases:
#   fused route against the float64 oracle (the push route gives the same figures to the digits shown)
#     bf16 gradients rel_l2 4.2e-3 (narrow lstm weight_ih_l0), rel_max 5.6e-3 (one_cell gru weight_hh_l0)    bounds 1e-2, 4e-2
#     bf16 dfeat worst row rel_l2 7.2e-3 (ragged lstm)                                                       bound 3e-2
#     fp32 gradients max norm 4.9e-7, dfeat 1.3e-6 (wide)                                                    bound 2e-4
#   fused route against ST_BPTT_FUSED=0
#     bf16 gradients rel_l2 3.6e-6, rel_max 2.2e-5 (bias sums), dfeat rows 6.9e-7; fp32 max norm 2.8e-7, dfeat 1.4e-6

V = 50


def _lens_ragged():
    """B = 37, batch sizes 37, 37, 33, 17, 16, 3 over the six steps"""
    lens = [6] * 3 + [5] * 13 + [4] * 1 + [3] * 16 + [2] * 4
    bs = [sum(1 for v in lens if v > t) for t in range(6)]
    assert bs == [37, 37, 33, 17, 16, 3], bs
    return lens


CASES = {
    #            E    H    L  lens
    "one_cell": (16, 16, 1, [2]),
    "ragged": (32, 32, 3, _lens_ragged()),
    "narrow": (16, 40, 2, [5, 4, 4, 2, 2]),
    "wide": (512, 512, 2, [3] * 20 + [2] * 13),
}


@functools.lru_cache(maxsize=None)
def _problem(case, cell, bf16):
    """(params, feat, cap, lens, oracle gradients, oracle dfeat): computed once per case, read-only afterwards"""
    Ed, Hd, L, lens = CASES[case]
    seed = 90 + sorted(CASES).index(case)
    params = R.init_decoder_params(Ed, Hd, V, L, cell, seed=seed)
    feat = torch.randn(len(lens), Ed, generator=torch.Generator().manual_seed(seed))
    if bf16:
        params, feat = _bf16_params(params), _bf16(feat)
    cap, lens = _captions(lens, V, seed)
    po = {k: v.double().requires_grad_(True) for k, v in params.items()}
    fo = feat.double().requires_grad_(True)
    R.gru_train_loss(po, fo, cap, lens, cell)[0].backward()
    return params, feat, cap, lens, {k: v.grad for k, v in po.items()}, fo.grad


def _run(case, cell, bf16):
    """one loss + backward on the GPU under the current ST_BPTT_FUSED: ({name: grad}, dfeat) as float64 on the host"""
    Ed, Hd, L, _ = CASES[case]
    params, feat, cap, lens, _, _ = _problem(case, cell, bf16)
    m = _decoder(cell, params, torch.bfloat16 if bf16 else torch.float32, Ed, Hd, V, L).train()
    fd = feat.cuda().requires_grad_(True)
    m.loss(fd, cap.cuda(), lens).backward()
    torch.cuda.synchronize()
    return {k: p.grad.detach().double().cpu() for k, p in m.named_parameters()}, fd.grad.detach().double().cpu()


def _compare(got, ref, bf16, tag):
    """every parameter gradient and d loss / d feat of `got` against `ref`, to the bounds of the storage type"""
    (gg, gf), (rg, rf) = got, ref
    for k in rg:
        if rg[k].abs().max() == 0:                    # embedding rows no caption uses, a 1 x 1 problem's unused pieces
            assert gg[k].abs().max() == 0, (tag, k)
            continue
        l2, mx = _rel_l2(gg[k], rg[k]), _rel_max(gg[k], rg[k])
        print(f"MEASURE {tag} {k}: rel_l2 {l2:.2e} rel_max {mx:.2e}")
        if bf16:
            assert l2 < GRAD_L2 and mx < GRAD_MAX, (tag, k, l2, mx)
        else:
            assert mx < FP32_REL, (tag, k, mx)
    row, mx = _row_l2(gf, rf), _rel_max(gf, rf)
    print(f"MEASURE {tag} dfeat: worst row rel_l2 {row:.2e} rel_max {mx:.2e}")
    if bf16:
        assert row < ROW_L2, (tag, row)
    else:
        assert mx < FP32_REL, (tag, mx)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cell", ["gru", "lstm"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_fused_bptt_matches_fp64_oracle_itself_and_the_push_route(case, cell, bf16, monkeypatch):
    _, _, _, _, og, of = _problem(case, cell, bf16)
    tag = f"{case} {cell} {'bf16' if bf16 else 'fp32'}"
    monkeypatch.setenv("ST_BPTT_FUSED", "1")
    fused = _run(case, cell, bf16)
    again = _run(case, cell, bf16)
    monkeypatch.setenv("ST_BPTT_FUSED", "0")
    push = _run(case, cell, bf16)
    _compare(fused, (og, of), bf16, f"{tag} fused/oracle")
    _compare(push, (og, of), bf16, f"{tag} push/oracle")
    # the recurrence, the dx0 GEMM and the weight-gradient GEMMs have no atomics: the same bits twice.  The embedding scatter
    # and the bias column sums add with fp32 atomics in an order that may change from call to call.
    for k in fused[0]:
        if "bias" in k or k.startswith("embeddings"):
            continue
        assert torch.equal(fused[0][k], again[0][k]), (tag, k)
    assert torch.equal(fused[1], again[1]), tag
    _compare(fused, push, bf16, f"{tag} fused/push")
