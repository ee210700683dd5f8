"""Beam search and attention maps of the soft-attention decoders (RNN_Attn.beam_search, sentence_index(return_alphas=True))
against beam_search.py:45-97 restated on the CPU and driven by the attention decoder's test branch (rnn_attn.py:77-94), with
each node's alpha carried as its `extras`."""
import numpy as np
import pytest
import torch

from oracle import restatement as R
from tests._util import load_fixture

pytestmark = pytest.mark.gpu
VOCAB = lambda w: {"<pad>": 0, "<start>": 1, "<end>": 2, "<unk>": 3}[w]   # vocab_builder.py:66-69


def _make(cell, params, dtype):
    from showtell_amd.rnn_attn import RNN_Attn
    from showtell_amd.rnn_attn_LSTM import RNN_Attn as RNN_Attn_LSTM
    V, E = params["embeddings.weight"].shape
    H = params["unit.weight_hh_l0"].shape[1]
    A, Fd = params["attn.encoder_att.weight"].shape
    L = R.num_layers_of(params)
    m = (RNN_Attn if cell == "gru" else RNN_Attn_LSTM)(E, Fd, A, H, V, L, dtype=dtype)
    m.load_state_dict(params)
    return m.cuda().eval()


def _sharpen(params, scale, boost):
    """As test_gpu_beam.py: a sharper vocabulary projection and a raised <end> logit, so that <end> competes.  The values are
    chosen per decoder so that the oracle's hypotheses run several tokens and some images end with none."""
    params = dict(params)
    params["linear.weight"] = params["linear.weight"] * scale
    b = params["linear.bias"].clone()
    b[2] += boost
    params["linear.bias"] = b
    return params


def attn_beam_callbacks(params, feat_row, cell):
    """beam_search.py callbacks for ONE image of the attention decoder.  feat_row (F, P).  The state is the flattened
    [h (L,H) ; c (L,H)]; generate is one test-branch step (rnn_attn.py:77-94) and returns alpha as the extras."""
    L = R.num_layers_of(params)
    H = params["unit.weight_hh_l0"].shape[1]
    lstm = cell != "gru"
    h0, c0 = R._attn_init(params, feat_row.unsqueeze(0), cell)                 # (L, 1, H)
    feat_pf = feat_row.t().unsqueeze(0)                                      # (1, P, F)

    def flat(h, c):
        s = h.transpose(0, 1).reshape(h.shape[1], L * H)
        if lstm:
            s = torch.cat([s, c.transpose(0, 1).reshape(c.shape[1], L * H)], 1)
        return s.numpy().astype(np.float32)

    def initial_state(_X):
        return flat(h0, c0)

    def generate(_X, Y_tm1, state_tm1):
        n = len(Y_tm1)
        s = torch.from_numpy(np.ascontiguousarray(state_tm1)).view(n, -1)
        h = s[:, :L * H].reshape(n, L, H).transpose(0, 1).contiguous()
        c = s[:, L * H:].reshape(n, L, H).transpose(0, 1).contiguous() if lstm else None
        z, alpha = R.attention_net(params, feat_pf.expand(n, -1, -1), h[-1])
        ez = z @ params["embed.weight"].t() + params["embed.bias"]
        x = torch.cat([params["embeddings.weight"][torch.from_numpy(Y_tm1.astype(np.int64))], ez], 1)
        top, h2, c2 = R.rnn_step(params, x, h, c, cell)
        p = torch.softmax(top @ params["linear.weight"].t() + params["linear.bias"], 1).numpy().astype(np.float32)
        return flat(h2, c2), p, [a for a in alpha.numpy().astype(np.float32)]

    return initial_state, generate


def oracle_beam(params, feat, cell, W, nh, T, start_id=1, end_id=2):
    """Per image: [(tokens, cost, alphas (len-1, P))] from the restated beam_search, extras walked through the parents."""
    out = []
    with torch.no_grad():
        for b in range(feat.shape[0]):
            init, gen = attn_beam_callbacks(params, feat[b], cell)
            res = []
            for hyp in R.beam_search(init, gen, [0], start_id, end_id, beam_width=W, num_hypotheses=nh, max_length=T):
                ext, n = [], hyp
                while n.parent is not None:
                    ext.append(n.extras)
                    n = n.parent
                res.append(([int(v) for v in hyp.to_sequence_of_values()], float(hyp.cum_cost), np.stack(ext[::-1])))
            out.append(res)
    return out


def oracle_greedy_alphas(params, feat, cell, steps=25, start_id=1):
    """R.attn_greedy (rnn_attn.py:120-145) keeping every step's alpha: (ids (B, steps), alphas (B, steps, P))."""
    B = feat.shape[0]
    with torch.no_grad():
        h, c = R._attn_init(params, feat, cell)
        feat_bpf = feat.transpose(1, 2)
        tok_emb = params["embeddings.weight"][torch.full((B,), start_id, dtype=torch.long)]
        ids, als = [], []
        for _ in range(steps):
            z, alpha = R.attention_net(params, feat_bpf, h[-1])
            ez = z @ params["embed.weight"].t() + params["embed.bias"]
            top, h, c = R.rnn_step(params, torch.cat([tok_emb, ez], 1), h, c, cell)
            tok = (top @ params["linear.weight"].t() + params["linear.bias"]).max(1)[1]
            ids.append(tok); als.append(alpha)
            tok_emb = params["embeddings.weight"][tok]
    return torch.stack(ids, 1), torch.stack(als, 1)


def _check_alpha_rows(alphas, tol):
    assert torch.isfinite(alphas).all()
    assert (alphas >= 0).all()
    assert torch.allclose(alphas.sum(-1), torch.ones(alphas.shape[:-1]), atol=tol)


def _compare(got, want, cost_tol, alpha_tol):
    assert len(got) == len(want)
    nonempty = 0
    for b, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), b
        nonempty += bool(g)
        for (gs, gc, ga), (ws, wc, wa) in zip(g, w):
            assert gs == ws, b
            assert abs(gc - wc) <= cost_tol * max(1.0, abs(wc)), (b, gc, wc)
            assert ga.dtype == torch.float32 and ga.shape == (len(gs) - 1, wa.shape[1]), (b, ga.shape)
            assert (ga - torch.from_numpy(wa)).abs().max().item() <= alpha_tol, b
            _check_alpha_rows(ga, 1e-5)
    return nonempty


CELLS = [("gru", "attn_gru_small.npz", 2), ("lstm", "attn_lstm_small.npz", 32)]
SMALL_SHARPEN = {"gru": (2.0, 0.0), "lstm": (2.0, 1.0)}
CONFIG3_SHARPEN = {"gru": (12.0, 1.3), "lstm": (12.0, 0.7)}


@pytest.mark.parametrize("cell,name,end_id", CELLS)
def test_width1_beam_is_the_reference_greedy_caption(cell, name, end_id):
    """W = 1 keeps one node: the reference's own greedy ids up to the first end_id (the LSTM fixture never emits 2)."""
    params, _, d = load_fixture(name)
    m = _make(cell, params, torch.float32)
    got = m.beam_search(torch.from_numpy(d["feat"]).cuda(), beam_width=1, max_length=25, end_id=end_id)
    for b, g in enumerate(d["greedy"].tolist()):
        want = [1] + g[:g.index(end_id) + 1]
        assert len(got[b]) == 1 and got[b][0][0] == want, (b, got[b], want)


@pytest.mark.parametrize("W", [3, 5])
@pytest.mark.parametrize("nh", [1, 3])
@pytest.mark.parametrize("cell,name", [c[:2] for c in CELLS])
def test_small_fixture_beam_tokens_costs_alphas_vs_oracle(cell, name, W, nh):
    params, _, d = load_fixture(name)
    params = _sharpen(params, *SMALL_SHARPEN[cell])
    m = _make(cell, params, torch.float32)
    feat = torch.from_numpy(d["feat"])
    got = m.beam_search(feat.cuda(), beam_width=W, num_hypotheses=nh, max_length=25, return_alphas=True)
    want = oracle_beam(params, feat, cell, W, nh, 25)
    assert _compare(got, want, 1e-4, 1e-5) >= 2
    plain = m.beam_search(feat.cuda(), beam_width=W, num_hypotheses=nh, max_length=25)
    assert [[(s, c) for s, c, _ in g] for g in got] == plain


def _config3(cell, B, seed=31):
    E, Fd, A, H, V, L = 512, 2048, 512, 512, 10000, 5
    params = _sharpen(R.init_decoder_params(E, H, V, L, cell, seed=seed, attn=dict(F=Fd, A=A)), *CONFIG3_SHARPEN[cell])
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(B, Fd, 49, generator=g).abs()                 # post-ReLU features are >= 0
    return params, feat, g


@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_config3_geometry_vs_oracle_and_batch_invariant(cell):
    """E = H = A = 512, F = 2048, P = 49, V = 10000, L = 5 (the config-3 decoder), 12 images, W = 5."""
    params, feat, _ = _config3(cell, 12)
    m = _make(cell, params, torch.float32)
    got = m.beam_search(feat.cuda(), beam_width=5, num_hypotheses=1, max_length=25, return_alphas=True)
    assert len(got) == 12
    S = (0, 1, 2, 4, 6, 7, 9, 11)
    want = oracle_beam(params, feat[list(S)], cell, 5, 1, 25)
    assert _compare([got[b] for b in S], want, 1e-3, 1e-4) >= 1
    assert sum(1 for h in got if h) >= 3
    sub = m.beam_search(feat[3:7].cuda(), beam_width=5, num_hypotheses=1, max_length=25, return_alphas=True)
    _same_search(sub, got[3:7])


def _same_search(a, b):
    """Equal token sequences; costs and alphas to the last bits (the cell GEMMs may tile 1280 rows differently from 60)."""
    assert len(a) == len(b)
    for a_, b_ in zip(a, b):
        assert len(a_) == len(b_)
        for (sa, ca, aa), (sb, cb, ab) in zip(a_, b_):
            assert sa == sb and abs(ca - cb) <= 1e-4 * max(1.0, abs(cb))
            assert (aa - ab).abs().max().item() <= 1e-5


def test_256_images_width5_fp32_batch_invariant_and_bf16_quality():
    """256 images x W = 5 (1280 beam rows): the fp32 search of the first 12 images equals the 12-image search of the test above
    image by image; the bf16 search is well formed and close to the fp32 one (BLEU-4 >= 0.9)."""
    params, feat12, g = _config3("gru", 12)
    feat = torch.cat([feat12, torch.randn(244, 2048, 49, generator=g).abs()], 0)
    m32 = _make("gru", params, torch.float32)
    small = m32.beam_search(feat12.cuda(), beam_width=5, num_hypotheses=3, max_length=25, return_alphas=True)
    big = m32.beam_search(feat.cuda(), beam_width=5, num_hypotheses=3, max_length=25, return_alphas=True)
    assert len(big) == 256
    _same_search(small, big[:12])
    m16 = _make("gru", params, torch.bfloat16)
    got = m16.beam_search(feat.cuda(), beam_width=5, num_hypotheses=3, max_length=25, return_alphas=True)
    assert len(got) == 256 and sum(1 for h in got if h) >= 32
    for hyp in got:
        costs = [c for _, c, _ in hyp]
        assert costs == sorted(costs)
        for s, c, a in hyp:
            assert s[0] == 1 and s[-1] == 2 and len(s) <= 26 and np.isfinite(c)
            assert a.shape == (len(s) - 1, 49)
            _check_alpha_rows(a, 1e-2)
    both = [b for b in range(256) if got[b] and big[b]]
    assert len(both) >= 32
    gts = {str(b): [" ".join(map(str, big[b][0][0]))] for b in both}
    res = {str(b): [" ".join(map(str, got[b][0][0]))] for b in both}
    assert R.bleu_corpus(gts, res, 4)[3] >= 0.9


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cell,name", [c[:2] for c in CELLS])
def test_greedy_attention_maps(cell, name, dtype):
    """sentence_index(return_alphas=True): the same ids as sentence_index(), and every step's alpha as the restated greedy loop
    computes it (bf16: up to the first step whose input token differs from the fp32 oracle's)."""
    params, _, d = load_fixture(name)
    if dtype == torch.bfloat16:
        params = {k: v.bfloat16().float() for k, v in params.items()}
    m = _make(cell, params, dtype)
    feat = torch.from_numpy(d["feat"])
    if dtype == torch.bfloat16:
        feat = feat.bfloat16().float()
    ids = m.sentence_index(feat.cuda(), VOCAB)
    ids2, alphas = m.sentence_index(feat.cuda(), VOCAB, return_alphas=True)
    assert torch.equal(ids, ids2)
    assert alphas.is_cuda and alphas.dtype == torch.float32 and alphas.shape == (4, 25, 49)
    ids_o, al_o = oracle_greedy_alphas(params, feat, cell)
    alphas = alphas.cpu()
    if dtype == torch.float32:
        assert torch.equal(ids.cpu(), ids_o)
        assert (alphas - al_o).abs().max().item() <= 1e-5
    else:
        for b in range(4):
            diff = (ids[b].cpu() != ids_o[b]).nonzero()
            last = int(diff[0]) if diff.numel() else 24          # alpha of step t depends on the tokens before t only
            assert (alphas[b, :last + 1] - al_o[b, :last + 1]).abs().max().item() <= 5e-2, b
    _check_alpha_rows(alphas, 1e-5 if dtype == torch.float32 else 1e-2)


def test_beam_search_argument_errors():
    from showtell_amd import ShowTellHipError
    params, _, d = load_fixture("attn_gru_small.npz")
    m = _make("gru", params, torch.float32)
    feat = torch.from_numpy(d["feat"])
    for W in (0, 9):
        with pytest.raises(ValueError):
            m.beam_search(feat.cuda(), beam_width=W)
    with pytest.raises(ValueError):
        m.beam_search(feat.cuda(), beam_width=3, max_length=0)
    with pytest.raises(ShowTellHipError):
        m.beam_search(feat, beam_width=3)
    with pytest.raises(ShowTellHipError):
        m.beam_search(torch.zeros(2, 48, 65, device="cuda"), beam_width=3)
    with pytest.raises(ShowTellHipError):
        m.sentence_index(feat, VOCAB, return_alphas=True)
