"""Pin of the oracle against the reference's own decoders on random shapes.

tests/golden/oracle_pin.npz holds the weights, inputs and outputs the reference's classes produced for these cases
(oracle/gen_golden.py pin); no reference code is needed to run the checks.
"""
import os

import numpy as np
import pytest
import torch

from oracle import restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_pin.npz")


@pytest.fixture(scope="module")
def ref():
    return np.load(GOLDEN)


def _case(ref, prefix):
    params = {k[len(prefix) + 2:]: torch.from_numpy(ref[k]) for k in ref.files if k.startswith(prefix + "p/")}
    return params, torch.from_numpy(ref[prefix + "feat"]), torch.from_numpy(ref[prefix + "caption"]), \
        [int(x) for x in ref[prefix + "lens"]]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_gru_forward_and_greedy_random_shapes(ref, seed):
    params, feat, cap, lens = _case(ref, "gru%d/" % seed)
    with torch.no_grad():
        np.testing.assert_allclose(R.rnn_forward(params, feat, cap, lens).numpy(),
                                   ref["gru%d/logits" % seed], atol=2e-5)
        assert torch.equal(R.rnn_greedy(params, feat), torch.from_numpy(ref["gru%d/greedy" % seed]))


def test_attn_gru_forward_random(ref):
    params, feat, cap, lens = _case(ref, "attn/")
    lo, ao = R.attn_forward(params, feat, cap, lens)
    np.testing.assert_allclose(lo.detach().numpy(), ref["attn/logits"], atol=2e-5)
    np.testing.assert_allclose(ao.detach().numpy(), ref["attn/alphas"], atol=2e-5)
