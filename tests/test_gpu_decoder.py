"""GPU parity of the decoder (st_rnn_forward / st_rnn_backward / st_cross_entropy /
st_rnn_greedy), the encoder head and the optimizers.

Golden vectors (tests/golden/*.npz) were produced by the reference's own classes; the
fp32 kernels must reproduce logits / loss / every gradient to 2e-4 of the tensor's scale
(fp32 sums re-associated by the MFMA tiling) and greedy token ids EXACTLY.
bf16 kernels (fp32 accumulation) are compared with the oracle at 4e-2 of the scale.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import restatement as R
from tests._util import load_fixture

pytestmark = pytest.mark.gpu


def _rel(got, ref):
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-12)).item()


def _make_sized(cell, params, dtype, E, H, V, L):
    from showtell_amd.rnn import RNN
    from showtell_amd.rnn_lstm import RNN as RNN_LSTM
    m = (RNN if cell == "gru" else RNN_LSTM)(E, H, V, L, dtype=dtype)
    m.load_state_dict({k: v.clone() for k, v in params.items()})
    return m.cuda().train()


def _make(cell, params, dtype):
    from showtell_amd.rnn import RNN
    from showtell_amd.rnn_lstm import RNN as RNN_LSTM
    V, E = params["embeddings.weight"].shape
    H = params["unit.weight_hh_l0"].shape[1]
    L = R.num_layers_of(params)
    m = (RNN if cell == "gru" else RNN_LSTM)(E, H, V, L, dtype=dtype)
    m.load_state_dict(params)
    return m.cuda()


@pytest.mark.parametrize("route", ["dropin", "fused"])
@pytest.mark.parametrize("cell,name", [("gru", "gru_small.npz"), ("lstm", "lstm_small.npz")])
def test_fp32_forward_loss_grads_match_reference_golden(cell, name, route):
    params, grads, d = load_fixture(name)
    m = _make(cell, params, torch.float32)
    feat = torch.from_numpy(d["feat"]).cuda().requires_grad_(True)
    cap, lens = torch.from_numpy(d["caption"]).cuda(), d["lens"].tolist()
    if route == "dropin":   # exactly main.py:145-151
        target = nn.utils.rnn.pack_padded_sequence(cap, lens, batch_first=True)[0]
        logits = m(feat, cap, lens)
        assert logits.shape == tuple(d["logits"].shape)
        assert _rel(logits, torch.from_numpy(d["logits"])) < 2e-4
        loss = nn.CrossEntropyLoss()(logits, target)
    else:
        loss = m.loss(feat, cap, lens)
    assert abs(loss.item() - float(d["loss"])) < 2e-5
    loss.backward()
    for k, g in grads.items():
        p = dict(m.named_parameters())[k]
        assert _rel(p.grad, g) < 2e-4, k
    # gradient w.r.t. the image feature: oracle autograd
    po = {k: v for k, v in params.items()}
    fo = torch.from_numpy(d["feat"]).requires_grad_(True)
    R.gru_train_loss(po, fo, torch.from_numpy(d["caption"]), lens, cell)[0].backward()
    assert _rel(feat.grad, fo.grad) < 2e-4


@pytest.mark.parametrize("cell,name", [("gru", "gru_small.npz"), ("lstm", "lstm_small.npz")])
def test_fp32_greedy_ids_exact(cell, name):
    params, _, d = load_fixture(name)
    m = _make(cell, params, torch.float32).eval()
    feat = torch.from_numpy(d["feat"]).cuda()
    ids = m.sentence_index(feat)
    assert ids.shape == (feat.shape[0], 25) and ids.dtype == torch.int64
    assert np.array_equal(ids.cpu().numpy(), d["greedy"])
    ids1 = m.sentence_index(feat[:1])
    assert ids1.shape == (25,)                                   # rnn.py:56 squeeze
    assert np.array_equal(ids1.cpu().numpy(), d["greedy_b1"])


@pytest.mark.parametrize("cell,name", [("gru", "gru_small.npz"), ("lstm", "lstm_small.npz")])
def test_greedy_paths_agree(cell, name):
    """st_rnn_greedy has three routes: keys per step with the embedding gather inside the layer-0 cell (steps <= 64), one
    re-armed key row (steps > 64), and materialised logits.  All must emit the same tokens."""
    import ctypes as C
    from showtell_amd._lib import check, lib
    from showtell_amd.rnn import _cp, _stream
    params, _, d = load_fixture(name)
    m = _make(cell, params, torch.float32).eval()
    feat = torch.from_numpy(d["feat"]).cuda()
    B = feat.shape[0]
    ids25, lg = m.sentence_index(feat, return_logits=True)                 # logits route
    assert np.array_equal(ids25.cpu().numpy(), d["greedy"])
    assert np.array_equal(lg.argmax(-1).cpu().numpy(), d["greedy"])
    prm, keep = m._c_params()
    nbytes = lib().st_rnn_greedy_workspace_bytes(C.byref(prm), B)
    for steps in (25, 64, 70):
        ws = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
        ids = torch.full((B, steps), -7, device="cuda", dtype=torch.long)
        check(lib().st_rnn_greedy(C.byref(prm), _cp(feat), B, steps, _cp(ws), nbytes, _cp(ids), None, _stream()), "st_rnn_greedy")
        got = ids.cpu().numpy()
        assert np.array_equal(got[:, :25], d["greedy"]), steps
        assert (got >= 0).all()
        if steps == 64:
            first64 = got
        if steps == 70:
            assert np.array_equal(got[:, :64], first64)


@pytest.mark.parametrize("B,V,H", [(128, 1000, 128), (130, 77, 64), (33, 4097, 128), (256, 520, 64), (5, 64, 64)])
def test_fused_argmax_grid_shapes(B, V, H):
    """The LDS-staged vocabulary arg-max runs on a 1-D grid in groups of 8 x ysplit blocks (row parts of one 64-entry slice
    on the same XCD, padding blocks in the last group): ragged V, V below one group, row counts that do and do not split,
    rows that are no multiple of 16.  Its tokens must equal the arg-max of the materialised logits (rnn.py:49-52)."""
    params = R.init_decoder_params(H, H, V, 2, "gru", seed=11)
    m = _make("gru", params, torch.float32).eval()
    feat = torch.randn(B, H, generator=torch.Generator().manual_seed(11)).cuda()
    ids_l, lg = m.sentence_index(feat, return_logits=True)
    ids_f = m.sentence_index(feat)
    assert ids_f.shape == (B, 25)
    assert np.array_equal(lg.argmax(-1).cpu().numpy(), ids_l.cpu().numpy())
    assert np.array_equal(ids_f.cpu().numpy(), ids_l.cpu().numpy())


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_bf16_forward_backward_close_to_oracle(cell):
    E, H, V, L, B = 64, 64, 200, 3, 16
    params = R.init_decoder_params(E, H, V, L, cell, seed=3)
    params = {k: v.bfloat16().float() for k, v in params.items()}   # both sides see bf16-representable weights
    m = _make(cell, params, torch.bfloat16)
    cap, lens = R.synthetic_captions(B, V, seed=3, mean=8, std=2, lo=4, hi=12)
    feat = (torch.randn(B, E, generator=torch.Generator().manual_seed(3))).bfloat16().float()
    po = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    lo, logits_o, _ = R.gru_train_loss(po, feat, cap, lens, cell)
    lo.backward()
    fd = feat.cuda().requires_grad_(True)
    logits = m(fd, cap.cuda(), lens)
    assert _rel(logits, logits_o) < 4e-2
    for p in m.parameters():
        p.grad = None
    loss = m.loss(fd, cap.cuda(), lens)
    assert abs(loss.item() - lo.item()) < 2e-2
    loss.backward()
    for k, p in m.named_parameters():
        assert _rel(p.grad, po[k].grad) < 4e-2, k


@pytest.mark.parametrize("cell,V,B", [("gru", 777, 9), ("lstm", 1500, 33), ("gru", 256, 4)])
def test_fused_vocab_cross_entropy_matches_launch_chain_and_oracle(cell, V, B, monkeypatch):
    """rnn.loss() in bf16 at H = 512 runs the vocabulary projection + cross entropy tile by tile without a logits tensor (csrc/vocab_ce.hip).
    Ragged sizes (V not a multiple of the 256-entry tile, tokens not a multiple of the 64-token tile, pad columns up to the leading dimension):
    loss and every gradient against the launch chain (ST_FUSED_CE=0: st_rnn_forward's logits + st_cross_entropy; it rounds the logits to bf16,
    the fused path keeps the fp32 accumulators) and against the fp32 oracle."""
    from showtell_amd._lib import lib
    E, H, L = 512, 512, 2
    params = R.init_decoder_params(E, H, V, L, cell, seed=5)
    params = {k: v.bfloat16().float() for k, v in params.items()}
    cap, lens = R.synthetic_captions(B, V, seed=5, mean=7, std=2, lo=3, hi=11)
    feat = (torch.randn(B, E, generator=torch.Generator().manual_seed(5))).bfloat16().float()
    out = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("ST_FUSED_CE", fused)
        m = _make_sized(cell, params, torch.bfloat16, E, H, V, L)
        fd = feat.cuda().requires_grad_(True)
        loss = m.loss(fd, cap.cuda(), lens)
        loss.backward()
        torch.cuda.synchronize()
        g = {k: p.grad.detach().float().cpu() for k, p in m.named_parameters()}
        g["feat"] = fd.grad.detach().float().cpu()
        out[fused] = (loss.item(), g)
    assert abs(out["1"][0] - out["0"][0]) < 2e-3
    for k in out["0"][1]:
        assert _rel(out["1"][1][k], out["0"][1][k]) < 2e-2, k
    po = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    fo = feat.clone().requires_grad_(True)
    lo, _, _ = R.gru_train_loss(po, fo, cap, lens, cell)
    lo.backward()
    assert abs(out["1"][0] - lo.item()) < 2e-2
    for k, v in po.items():
        assert _rel(out["1"][1][k], v.grad) < 4e-2, k


def test_fused_vocab_cross_entropy_three_sgd_steps_track_the_launch_chain(monkeypatch):
    """Three SGD steps of the bf16 GRU decoder at H = 512 through rnn.loss() with the fused vocabulary projection + cross entropy against the
    same three steps on the launch chain: losses and final weights agree to bf16-path tolerance (the fused path keeps fp32 logits)."""
    from showtell_amd import optim
    E, H, V, L, B = 512, 512, 1200, 2, 24
    params = R.init_decoder_params(E, H, V, L, "gru", seed=21)
    cap, lens = R.synthetic_captions(B, V, seed=21, mean=8, std=2, lo=4, hi=12)
    feat = torch.randn(B, E, generator=torch.Generator().manual_seed(21)).cuda()
    res = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("ST_FUSED_CE", fused)
        m = _make_sized("gru", params, torch.bfloat16, E, H, V, L)
        opt = optim.SGD(m.parameters(), lr=0.05, momentum=0.9)
        losses = []
        for _ in range(3):
            opt.zero_grad()
            loss = m.loss(feat, cap.cuda(), lens)
            loss.backward()
            opt.step()
            losses.append(loss.item())
        res[fused] = (losses, {k: v.detach().float().cpu().clone() for k, v in m.state_dict().items()})
    for a, b in zip(res["1"][0], res["0"][0]):
        assert abs(a - b) < 5e-3 * max(1.0, abs(b))
    assert res["1"][0][-1] < res["1"][0][0]                    # the loss goes down
    for k in res["0"][1]:
        assert _rel(res["1"][1][k], res["0"][1][k]) < 2e-2, k


def test_fp32_full_size_gru_step_matches_oracle():
    """BASELINE config shape: E=H=512, L=5, V=10000, B=128 synthetic captions."""
    E, H, V, L, B = 512, 512, 10000, 5, 128
    params = R.init_decoder_params(E, H, V, L, "gru", seed=1)
    m = _make("gru", params, torch.float32)
    cap, lens = R.synthetic_captions(B, V, seed=1)
    feat = torch.randn(B, E, generator=torch.Generator().manual_seed(1))
    po = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    lo, _, _ = R.gru_train_loss(po, feat, cap, lens, "gru")
    lo.backward()
    loss = m.loss(feat.cuda().requires_grad_(True), cap.cuda(), lens)
    assert abs(loss.item() - lo.item()) < 1e-4
    loss.backward()
    for k, p in m.named_parameters():
        assert _rel(p.grad, po[k].grad) < 5e-4, k
    # size-independent property: d(loss)/d(linear.bias) sums to zero (softmax - onehot rows sum to 0)
    assert abs(m.linear.bias.grad.sum().item()) < 1e-5
    # greedy ids at full size: exact against the oracle
    with torch.no_grad():
        ids_o = R.rnn_greedy(params, feat[:16], "gru")
    ids = m.eval().sentence_index(feat[:16].cuda())
    assert torch.equal(ids.cpu(), ids_o)


def test_edge_cases_single_sample_equal_lengths_and_errors():
    from showtell_amd import ShowTellHipError
    params = R.init_decoder_params(32, 48, 40, 2, "gru", seed=4)
    m = _make("gru", params, torch.float32)
    # B=1, length 3
    cap = torch.tensor([[1, 7, 2]])
    feat = torch.randn(1, 32, generator=torch.Generator().manual_seed(2))
    ref = R.rnn_forward(params, feat, cap, [3])
    assert _rel(m(feat.cuda(), cap.cuda(), [3]), ref) < 2e-4
    # all lengths equal (no ragged tail), padded caption wider than the longest length
    cap = torch.tensor([[1, 5, 6, 2, 0, 0], [1, 9, 8, 2, 0, 0]])
    feat = torch.randn(2, 32, generator=torch.Generator().manual_seed(3))
    ref = R.rnn_forward(params, feat, cap, [4, 4])
    assert _rel(m(feat.cuda(), cap.cuda(), [4, 4]), ref) < 2e-4
    with pytest.raises(RuntimeError):
        m(feat.cuda(), cap.cuda(), [3, 4])                      # unsorted lengths (pack_padded_sequence rule)
    with pytest.raises(ShowTellHipError):
        m.cpu()(feat, cap, [4, 4])                              # no CPU fallback


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("train", [True, False])
def test_encoder_head_linear_bn1d(dtype, train):
    from showtell_amd.head import linear_bn1d
    g = torch.Generator().manual_seed(8)
    B, F, E = 32, 256, 64
    lin, bn = nn.Linear(F, E), nn.BatchNorm1d(E, momentum=0.01)
    lin.weight.data.normal_(0, 0.05, generator=g)
    bn.weight.data.uniform_(0.5, 1.5, generator=g); bn.bias.data.normal_(0, 0.1, generator=g)
    bn.running_mean.normal_(0, 0.1, generator=g); bn.running_var.uniform_(0.5, 1.5, generator=g)
    x = torch.randn(B, F, generator=g)
    if dtype == torch.bfloat16:
        lin.weight.data = lin.weight.data.bfloat16().float(); x = x.bfloat16().float()
    import copy
    lin_d, bn_d = copy.deepcopy(lin).cuda(), copy.deepcopy(bn).cuda()
    lin.train(train); bn.train(train)
    y_ref = bn(lin(x))
    w = torch.randn(B, E, generator=g)
    (y_ref * w).sum().backward()
    y = linear_bn1d(x.cuda(), lin_d, bn_d, train, dtype)
    (y * w.cuda()).sum().backward()
    tol = 2e-4 if dtype == torch.float32 else 3e-2
    assert _rel(y, y_ref) < tol
    for a, b in ((lin_d.weight, lin.weight), (lin_d.bias, lin.bias), (bn_d.weight, bn.weight), (bn_d.bias, bn.bias)):
        if train and a is lin_d.bias:
            # batch-stat BN makes d(loss)/d(linear.bias) analytically ZERO (the reference value is fp32 noise);
            # bound ours by the rounding of the 32 dz terms that cancel (each O(1)) instead of a relative test
            assert a.grad.abs().max().item() < (1e-4 if dtype == torch.float32 else 5e-2)
            continue
        assert _rel(a.grad, b.grad) < tol
    assert _rel(bn_d.running_mean, bn.running_mean) < tol and _rel(bn_d.running_var, bn.running_var) < tol
    assert int(bn_d.num_batches_tracked) == int(bn.num_batches_tracked)


@pytest.mark.parametrize("kind", ["sgd", "sgd0", "adam"])
def test_optimizers_match_torch(kind):
    from showtell_amd import optim
    g = torch.Generator().manual_seed(12)
    shapes = [(50, 64), (192, 64), (192,), (7,), (33, 5)]
    ref = [nn.Parameter(torch.randn(*s, generator=g)) for s in shapes]
    dev = [nn.Parameter(p.data.clone().cuda()) for p in ref]
    if kind == "sgd":
        o_ref, o_dev = torch.optim.SGD(ref, lr=0.01, momentum=0.9), optim.SGD(dev, lr=0.01, momentum=0.9)
    elif kind == "sgd0":
        o_ref, o_dev = torch.optim.SGD(ref, lr=0.05), optim.SGD(dev, lr=0.05)
    else:
        o_ref, o_dev = torch.optim.Adam(ref, lr=1e-3), optim.Adam(dev, lr=1e-3)
    for step in range(4):
        o_ref.zero_grad(); o_dev.zero_grad()
        for p, q in zip(ref, dev):
            gr = torch.randn(p.shape, generator=g)
            p.grad = gr.clone(); q.grad.copy_(gr)
        o_ref.step(); o_dev.step()
        for p, q in zip(ref, dev):
            np.testing.assert_allclose(q.detach().cpu().numpy(), p.detach().numpy(), rtol=2e-5, atol=2e-6)
    # the bf16 shadow follows the parameters
    for q in dev:
        assert torch.equal(q._st_shadow.float().cpu(), q.detach().bfloat16().float().cpu())


@pytest.mark.parametrize("cell", ["gru", "lstm"])
@pytest.mark.parametrize("B,L,V", [(128, 5, 10000), (8, 5, 10000), (33, 5, 10000), (256, 5, 10000), (64, 3, 9000), (40, 1, 12000), (16, 5, 777)])
def test_pipelined_greedy_decoder_equals_launch_chain(B, L, V, cell, monkeypatch):
    """rnn.py:37-58 / LSTM/rnn_lstm.py:35-57 at the BASELINE decoder shape (E = H = 512, bf16): the persistent layer-per-XCD decoder (csrc/decode_pipe.hip)
    must return the launch chain's token ids bit for bit -- same MFMA order, same gate function, same arg-max keys -- for full and
    ragged chains (B not a multiple of 32), fewer layers (more vocabulary XCDs) and other vocabulary sizes; and the fp32 / oracle
    agreement the launch chain is tested for carries over."""
    from showtell_amd.rnn import RNN
    from showtell_amd.rnn_lstm import RNN as RNN_LSTM
    E = H = 512
    sd = R.init_decoder_params(E, H, V, L, cell, seed=11 + B)
    sd["linear.weight"] *= 6.0
    if cell == "lstm":        # a default-initialised LSTM stack decodes to one constant token: give its gates some swing
        for k in sd:
            if k.startswith("unit.weight"):
                sd[k] = sd[k] * 5.0
    m = (RNN if cell == "gru" else RNN_LSTM)(E, H, V, L, dtype=torch.bfloat16); m.load_state_dict(sd); m = m.cuda().eval()
    feat = torch.randn(B, E, generator=torch.Generator().manual_seed(B)).cuda()
    from showtell_amd._lib import lib
    from tests.test_gpu_decoder_bench_shape import assert_pipe_ran
    monkeypatch.setenv("ST_DECODE_PIPE", "0")
    ids_chain = m.sentence_index(feat)
    assert lib().st_rnn_greedy_last_route() == 1
    monkeypatch.setenv("ST_DECODE_PIPE", "1")
    ids_pipe = m.sentence_index(feat)
    assert_pipe_ran()                                      # the pipe ran: otherwise the chain is compared with itself
    ids_pipe2 = m.sentence_index(feat)                     # a second run on a reused workspace (stale buffers must not matter)
    assert_pipe_ran()
    torch.cuda.synchronize()
    assert ids_pipe.shape == ids_chain.shape == (B, 25)
    assert torch.equal(ids_pipe, ids_chain)
    assert torch.equal(ids_pipe2, ids_chain)
    assert ids_chain.min().item() >= 0 and ids_chain.max().item() < V
    assert len(torch.unique(ids_chain)) > 5                # not a degenerate decode
