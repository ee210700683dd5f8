"""GPU parity of the two beam decoders against vectors produced by the reference itself
(rnn.py:60-108 via RNN.sentence_index(beam_size=k); beam_search.py driven by the reference's RNN)."""
import numpy as np
import pytest
import torch

from oracle import restatement as R
from tests._util import load_fixture
from tests.test_gpu_decoder import _make

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k", [1, 3, 5])
def test_quirky_beam_ids_exact_vs_reference(k):
    params, _, d = load_fixture("gru_small.npz")
    m = _make("gru", params, torch.float32).eval()
    feat = torch.from_numpy(d["feat"])[:1].cuda()
    ids = m.sentence_index(feat, beam_size=k)
    assert ids.shape == (25,) and ids.dtype == torch.int64
    assert np.array_equal(ids.cpu().numpy(), d[f"qbeam{k}"])
    with pytest.raises(ValueError):
        m.sentence_index(torch.from_numpy(d["feat"])[:2].cuda(), beam_size=k)   # bs=1 only (rnn.py:60)


@pytest.mark.parametrize("bw,nh", [(5, 3), (4, 1)])
def test_beam_search_sequences_exact_vs_reference(bw, nh):
    params, _, d = load_fixture("beam_small.npz")
    m = _make("gru", params, torch.float32).eval()
    feat = torch.from_numpy(d["feat"]).cuda()
    out = m.beam_search(feat, beam_width=bw, num_hypotheses=nh, max_length=int(d[f"bw{bw}_maxlen"]))
    assert len(out) == feat.shape[0]
    for b, hyp in enumerate(out):
        lens = d[f"bw{bw}_len"][b]
        assert len(hyp) == int((lens > 0).sum())            # [] when nothing completed (beam_search.py:69-79)
        for i, (seq, cost) in enumerate(hyp):
            assert seq == d[f"bw{bw}_seq"][b, i, :lens[i]].tolist()
            assert abs(cost - d[f"bw{bw}_cost"][b, i]) < 1e-3


def test_beam_search_full_size_matches_oracle_and_is_batch_invariant():
    """E=H=512, L=5, V=10000 (BASELINE config 5 shape, fewer images): ids equal the oracle's, and an image's
    result does not depend on what else is in the batch."""
    E, H, V, L, B = 512, 512, 10000, 5, 12
    params = R.init_decoder_params(E, H, V, L, "gru", seed=6)
    params["linear.weight"] = params["linear.weight"] * 12.0      # sharpen so that <end> competes (see gen_golden.gen_beam)
    params["linear.bias"][2] += 1.5
    m = _make("gru", params, torch.float32).eval()
    feat = torch.randn(B, E, generator=torch.Generator().manual_seed(6))
    got = m.beam_search(feat.cuda(), beam_width=5, num_hypotheses=1, max_length=25)
    nonempty = 0
    for b in range(B):
        with torch.no_grad():
            init, gen = R.gru_beam_callbacks(params, feat[b])
            hyp = R.beam_search(init, gen, [0], 1, 2, beam_width=5, num_hypotheses=1, max_length=25)
        assert len(got[b]) == len(hyp)
        if hyp:
            nonempty += 1
            assert got[b][0][0] == hyp[0].to_sequence_of_values()
            assert got[b][0][0][0] == 1 and got[b][0][0][-1] == 2
    assert nonempty >= 3
    sub = m.beam_search(feat[3:7].cuda(), beam_width=5, num_hypotheses=1, max_length=25)
    assert [h[0][0] if h else None for h in sub] == [h[0][0] if h else None for h in got[3:7]]


def test_beam_search_256_images_beam5_config5_size():
    """BASELINE configs[4] at its real size: 256 images x beam 5 = 1280-row cells (the `MT` tall-cell path that shares weight
    fragments across row tiles) and st_beam_select over 256 image slots.  fp32 kernels: (i) the first 12 images of the 256-image
    search equal the 12-image search of the test above image by image (batch invariance across the cell-size change), (ii) eight
    images spread over the batch equal the CPU oracle (beam_search.py:45-97 restated), (iii) every non-empty hypothesis starts
    with <start>, ends with <end> and is at most max_length long."""
    E, H, V, L, B = 512, 512, 10000, 5, 256
    params = R.init_decoder_params(E, H, V, L, "gru", seed=6)
    params["linear.weight"] = params["linear.weight"] * 12.0
    params["linear.bias"][2] += 1.5
    m = _make("gru", params, torch.float32).eval()
    g = torch.Generator().manual_seed(6)
    feat12 = torch.randn(12, E, generator=g)                       # the same 12 images as the test above
    feat = torch.cat([feat12, torch.randn(B - 12, E, generator=g)], 0)
    got = m.beam_search(feat.cuda(), beam_width=5, num_hypotheses=1, max_length=25)
    assert len(got) == B
    small = m.beam_search(feat12.cuda(), beam_width=5, num_hypotheses=1, max_length=25)
    assert [h[0][0] if h else None for h in small] == [h[0][0] if h else None for h in got[:12]]
    for a_, b_ in zip(small, got[:12]):
        if a_:
            assert abs(a_[0][1] - b_[0][1]) < 1e-3
    checked = 0
    for b in (0, 5, 40, 97, 128, 191, 230, 255):
        with torch.no_grad():
            init, gen = R.gru_beam_callbacks(params, feat[b])
            hyp = R.beam_search(init, gen, [0], 1, 2, beam_width=5, num_hypotheses=1, max_length=25)
        assert len(got[b]) == len(hyp), b
        if hyp:
            checked += 1
            assert got[b][0][0] == hyp[0].to_sequence_of_values(), b
    assert checked >= 2
    done = [h[0][0] for h in got if h]
    assert len(done) >= B // 8
    assert all(s_[0] == 1 and s_[-1] == 2 and len(s_) <= 26 for s_ in done)


def test_bf16_greedy_bleu4_vs_fp32_oracle():
    """BASELINE config 5 quality gate at the full decoder shape: 25-token greedy captions of the bf16 kernels against the fp32
    CPU oracle (rnn.py:37-58) on the same weights, scored with the reference's BLEU (corpus BLEU-4 >= 0.9: random-init
    weights make near-ties common, bf16 rounding flips a few tokens); the fp32 kernels must give the oracle's ids exactly."""
    from showtell_amd.rnn import RNN
    E = H = 512
    L, V = 5, 10000
    sd = R.init_decoder_params(E, H, V, L, "gru", seed=6)
    sd["linear.weight"] *= 12.0
    sd["linear.bias"][2] += 1.5
    fq = torch.randn(8, E, generator=torch.Generator().manual_seed(6))
    with torch.no_grad():
        g_ref = R.rnn_greedy(sd, fq)
    r32 = RNN(E, H, V, L, dtype=torch.float32); r32.load_state_dict(sd); r32 = r32.cuda().eval()
    r16 = RNN(E, H, V, L, dtype=torch.bfloat16); r16.load_state_dict(sd); r16 = r16.cuda().eval()
    assert torch.equal(r32.sentence_index(fq.cuda()).cpu(), g_ref)
    g_hip = r16.sentence_index(fq.cuda()).cpu()
    gts = {str(b): [" ".join(map(str, g_ref[b].tolist()))] for b in range(8)}
    res = {str(b): [" ".join(map(str, g_hip[b].tolist()))] for b in range(8)}
    assert R.bleu_corpus(gts, res, 4)[3] >= 0.9


@pytest.mark.parametrize("V,ldl", [(5003, 5008), (2048, 2048), (2047, 2048), (37, 40)])
@pytest.mark.parametrize("k", [1, 5, 8, 12])
def test_softmax_topk_kernels_against_torch(k, V, ldl):
    """st_softmax_topk: the threshold form (k <= 8 and k * 256 <= V) and the general form (k = 12, or a shorter row) against
    torch -- indices exact including ties (first index wins, as torch.sort(stable) on the negated row), probabilities to float32
    rounding; raw mode returns logits.  V = 2048 with k = 8 is the first row length on the threshold kernel (exactly k * 256),
    2047 falls to the general kernel, and at V = 37 most threads hold no element, so the empty index takes part in every merge."""
    import ctypes as C
    from showtell_amd._lib import check, lib
    from showtell_amd.rnn import _cp, _stream
    torch.manual_seed(3)
    n = 37
    x = torch.randn(n, ldl, device="cuda")
    x[:, ::7] = x[:, 3:4]                                # many exact ties, some of them at the top
    x[5, :V] = 0.25                                      # a constant row: indices 0 .. k-1
    x[6, :V] = -float("inf"); x[6, 17] = 1.0             # one finite entry
    for raw in (0, 1):
        p = torch.empty(n, k, device="cuda")
        i = torch.empty(n, k, device="cuda", dtype=torch.long)
        check(lib().st_softmax_topk(_cp(x), ldl, n, V, k, _cp(p), _cp(i), raw, _stream()), "st_softmax_topk")
        row = x[:, :V]
        order = torch.sort(-row, dim=1, stable=True).indices[:, :k]
        keep = torch.ones(n, dtype=torch.bool); keep[6] = False      # row 6: only the first index is defined by a finite value
        assert torch.equal(i[keep.cuda()], order[keep.cuda()])
        assert int(i[6, 0]) == 17
        ref = torch.gather(row if raw else torch.softmax(row, 1), 1, order)
        assert torch.allclose(p[keep.cuda()], ref[keep.cuda()], rtol=2e-6, atol=1e-9)


@pytest.mark.parametrize("bw,nh,dtype", [(5, 3, torch.float32), (4, 1, torch.float32), (5, 1, torch.bfloat16), (8, 2, torch.float32), (9, 1, torch.float32)])
def test_beam_search_device_selection_equals_host_bookkeeping(bw, nh, dtype):
    """The device-side fringe selection (st_beam_select, one host round trip per search) against the host bookkeeping that
    replays the reference's lists: same hypotheses, sequences and order; costs to float32 rounding of -log p.  bw=9 exceeds the
    W*k <= 64 limit of the kernel and must fall back to the host path by itself."""
    from showtell_amd.beam import beam_search, beam_search_host
    E, H, V, L, B = 128, 128, 600, 3, 40
    params = R.init_decoder_params(E, H, V, L, "gru", seed=9)
    params["linear.weight"] = params["linear.weight"] * 10.0
    params["linear.bias"][2] += 1.0
    m = _make("gru", params, dtype).eval()
    feat = torch.randn(B, E, generator=torch.Generator().manual_seed(9)).cuda()
    dev = beam_search(m, feat, beam_width=bw, num_hypotheses=nh, max_length=25)
    host = beam_search_host(m, feat, beam_width=bw, num_hypotheses=nh, max_length=25)
    assert len(dev) == len(host) == B
    assert sum(1 for h in host if h) >= B // 4
    for d_, h_ in zip(dev, host):
        assert [s for s, _ in d_] == [s for s, _ in h_]
        for (_, cd), (_, ch) in zip(d_, h_):
            assert abs(cd - ch) <= 1e-5 * max(1.0, abs(ch))
