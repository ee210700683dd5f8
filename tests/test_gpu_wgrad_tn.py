"""The decoder's parameter gradients as token contractions of the operands as they lie (ST_WGRAD_TN=1, the default for bf16:
st_gemm_tn_batch, csrc/gemm_tn.hip) against the float64 oracle, against the route they replace (ST_WGRAD_TN=0: K-major copies,
st_gemm_nt, bias sums with fp32 atomics) and against themselves: one loss + backward of the plain decoder on the `narrow`
(E 16, H 40, L 2: in0 != H is a group with its own N), `ragged` (B 37, batch sizes 37, 37, 33, 17, 16, 3: h_{t-1} gathered
through prev_row) and `wide` (H 512, L 2, B 33: full tiles, the fused cross entropy's padded dlogits) cases of
tests/test_gpu_rnn_bptt_fused.py, GRU and LSTM.

Bounds: GRAD_L2 / GRAD_MAX / ROW_L2 of tests/test_gpu_decoder_bench_shape.py for both routes against the oracle and for the new
route against the old one (identical bf16 operands, fp32 summation order differs).  The new route has no atomics in any weight or
bias gradient, so two calls give the same bits (the embedding scatter keeps its atomics).  fp32 does not change route: the same bits
under ST_WGRAD_TN=1 and =0 (weights; its bias sums and embedding scatter add with atomics in either).
"""
import pytest
import torch

from tests.test_gpu_rnn_bptt_fused import _compare, _problem, _run

pytestmark = pytest.mark.gpu

# MEASURED (MI355X), worst over the 6 cases:
#   either route against the float64 oracle (the same figures to the digits shown)
#     gradients rel_l2 4.2e-3 (narrow lstm weight_ih_l0), rel_max 5.0e-3 (narrow lstm weight_hh_l0)      bounds 1e-2, 4e-2
#     dfeat worst row rel_l2 7.2e-3 (ragged lstm)                                                           bound 3e-2
#   new route against ST_WGRAD_TN=0
#     weight gradients equal to the bit (both routes feed v_mfma_f32_16x16x32_bf16 the tokens in the same order), bias gradients
#     rel_max 1.1e-8 (wide gru bias_ih_l1: ordered sums against atomics), embeddings 2.3e-7 (atomics in both), dfeat equal


@pytest.mark.parametrize("cell", ["gru", "lstm"])
@pytest.mark.parametrize("case", ["narrow", "ragged", "wide"])
def test_token_contraction_matches_fp64_oracle_the_old_route_and_itself(case, cell, monkeypatch):
    _, _, _, _, og, of = _problem(case, cell, True)
    tag = f"{case} {cell} bf16"
    monkeypatch.setenv("ST_WGRAD_TN", "1")
    new = _run(case, cell, True)
    again = _run(case, cell, True)
    monkeypatch.setenv("ST_WGRAD_TN", "0")
    old = _run(case, cell, True)
    _compare(new, (og, of), True, f"{tag} tn/oracle")
    _compare(old, (og, of), True, f"{tag} nt/oracle")
    _compare(new, old, True, f"{tag} tn/nt")
    for k in new[0]:
        if k.startswith("embeddings"):
            continue
        assert torch.equal(new[0][k], again[0][k]), (tag, k)
    assert torch.equal(new[1], again[1]), tag


@pytest.mark.parametrize("cell", ["gru", "lstm"])
@pytest.mark.parametrize("case", ["narrow", "wide"])
def test_fp32_keeps_its_route(case, cell, monkeypatch):
    monkeypatch.setenv("ST_WGRAD_TN", "1")
    on = _run(case, cell, False)
    monkeypatch.setenv("ST_WGRAD_TN", "0")
    off = _run(case, cell, False)
    for k in on[0]:
        if "bias" in k or k.startswith("embeddings"):
            continue
        assert torch.equal(on[0][k], off[0][k]), (case, cell, k)
    assert torch.equal(on[1], off[1]), (case, cell)
