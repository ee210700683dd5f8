"""beam.replay_hypotheses (host side of the device beam searches) on hand-made records: token sequences, costs, harvest
order and, for the attention decoder, the extras of each node -- the alpha of its PARENT's row one iteration earlier."""
import numpy as np
import torch

from showtell_amd.beam import replay_hypotheses


def _records():
    T, B, W, P = 3, 2, 2, 4
    tok = np.zeros((T + 1, B, W), np.int64)
    cost = np.full((T + 1, B, W), np.inf, np.float32)
    par = np.full((T + 1, B, W), -1, np.int32)
    end = np.zeros((T, B, W), np.uint8)
    tok[0, :, 0], cost[0, :, 0] = 1, 0.0
    tok[1], par[1], cost[1] = [[5, 6], [7, 8]], [[0, 0], [0, 0]], [[1, 2], [1, 2]]
    tok[2], par[2], cost[2] = [[2, 9], [9, 2]], [[1, 0], [0, 1]], [[3, 4], [3, 5]]
    tok[3], par[3], cost[3] = [[2, 2], [2, 2]], [[1, 1], [0, 0]], [[6, 7], [6, 7]]   # ended on the last iteration: never harvested
    end[2] = [[1, 0], [0, 1]]
    alphas = (100 * np.arange(T)[:, None, None] + 10 * np.arange(B * W)[None, :, None] + np.arange(P)).astype(np.float32)
    return tok, cost, par, end, alphas


def test_replay_sequences_costs_and_parent_extras():
    tok, cost, par, end, alphas = _records()
    got = replay_hypotheses(tok, cost, par, end, 3, alphas)
    assert [[(s, c) for s, c, _ in h] for h in got] == [[([1, 6, 2], 3.0)], [([1, 8, 2], 5.0)]]
    # image 0: node (2, 0) has parent slot 1 -> alphas[1][0*2 + 1]; node (1, 1) has parent slot 0 -> alphas[0][0]
    assert torch.equal(got[0][0][2], torch.from_numpy(np.stack([alphas[0, 0], alphas[1, 1]])))
    # image 1: node (2, 1) has parent slot 1 -> alphas[1][1*2 + 1]; node (1, 1) has parent slot 0 -> alphas[0][2]
    assert torch.equal(got[1][0][2], torch.from_numpy(np.stack([alphas[0, 2], alphas[1, 3]])))
    assert got[0][0][2].dtype == torch.float32


def test_replay_without_extras_and_hypothesis_order():
    tok, cost, par, end, _ = _records()
    end[1] = [[1, 0], [0, 0]]                     # image 0 also harvests node (1, 0) = [1, 5] at cost 1
    got = replay_hypotheses(tok, cost, par, end, 3)
    assert got == [[([1, 5], 1.0), ([1, 6, 2], 3.0)], [([1, 8, 2], 5.0)]]
    assert replay_hypotheses(tok, cost, par, end, 1) == [[([1, 5], 1.0)], [([1, 8, 2], 5.0)]]
    assert replay_hypotheses(tok, cost, par, np.zeros_like(end), 2) == [[], []]
