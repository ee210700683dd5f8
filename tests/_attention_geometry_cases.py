"""Cases, inputs, launch arithmetic and seeded faults for tests/test_gpu_attention_geometry.py (GPU) and
tests/test_attention_geometry_inputs.py (CPU).  Nothing here needs a GPU.

  CASES          the case table: the smallest shapes at which the attention kernels take each of their code paths
  problem        (params, feat, cap, lens) of one (case, cell, dtype), bf16-representable for the bf16 kernels
  paths          pure-Python mirror of attn_fwd_launch / attn_bwd_launch / attn_beam_fwd_launch (csrc/attn_kernels.hip) and of
                 make_plan's Np (csrc/attn.cpp)
  train_copy     a copy of R.attn_forward / R.attn_train_loss with encoder_att hoisted (d att1 readable) and the seeded faults
  storage_distance what bf16 storage alone does to each gradient: the copy with rounding at make_plan's storage points
  beam_step_copy a copy of R.attn_beam_step_bf16_storage with the slot fault
  greedy_walk    the storage restatement at W = 1 walked along given tokens (its own arg-max when none are given)
  beam_floor     tests/_beam_oracle.py's beam_distance, fp32 against float64 arithmetic, on given inputs
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import restatement as R
from tests._beam_oracle import StepOracle, beam_distance  # noqa: F401
from tests._util import _bf16

V = 50
STEPS = 25          # RNN_Attn.cap_max_size
BEAM_T = 8          # max_length of the beam searches
BEAM_IMAGES = 3     # images of a beam search on the GPU
FLOOR_IMAGES = 512  # images the floors of the beam bounds are measured on (the GPU's 3 are the first 3 of them)
BEAM_WIDTHS = (2, 4, 6, 7)
BEAM_CASES = ("full_wave", "tokens_gt_pixels")
GREEDY_CASES = ("full_wave", "tokens_gt_pixels", "wide_att", "wide_feat")


def _lens_many_rows():
    """520 captions of lengths 2..5, descending: steps 0 and 1 have 520 rows, the later ones fewer than 512"""
    rng = np.random.RandomState(520)
    lens = sorted([int(v) for v in rng.randint(2, 6, size=520)], reverse=True)
    assert set(lens) == {2, 3, 4, 5}
    return lens


# `scale` multiplies attn.full_att.weight; seed and scale are chosen so that the peakedness conditions of
# test_attention_geometry_inputs.py hold with room (values there)
CASES = {
    #                    E    F     A     H   P   L  lens
    "one_pixel": dict(E=16, F=8, A=8, H=16, P=1, L=1, lens=[2], seed=3, scale=8.0),
    "full_wave": dict(E=32, F=48, A=40, H=64, P=64, L=2, lens=[9, 7, 7, 4, 2], seed=3, scale=8.0),
    "tokens_gt_pixels": dict(E=32, F=64, A=32, H=32, P=4, L=2, lens=[12, 11, 9, 9, 8, 6, 5], seed=4, scale=10.0),
    "odd": dict(E=24, F=40, A=24, H=40, P=33, L=3, lens=[6, 6, 5, 3, 3, 1], seed=3, scale=8.0),
    "wide_att": dict(E=64, F=256, A=1032, H=64, P=17, L=1, lens=[5, 4, 4, 2], seed=3, scale=8.0),
    "wide_feat": dict(E=16, F=4104, A=16, H=16, P=9, L=1, lens=[3, 2], seed=3, scale=16.0),
    "many_rows": dict(E=16, F=48, A=40, H=16, P=10, L=1, lens=_lens_many_rows(), seed=5, scale=9.0),
}


def features(B, Fd, P, seed, bf16):
    """(B, F, P) post-ReLU features |randn| with a per-(sample, pixel) gain, as tests/test_gpu_attention_bench_shape.py's"""
    g = torch.Generator().manual_seed(seed)
    gain = 0.75 + 0.5 * torch.rand(B, 1, P, generator=g)
    x = torch.randn(B, Fd, P, generator=g).abs() * gain
    return _bf16(x) if bf16 else x


def captions(lens, seed):
    """zero-padded [1] + randint(4, V) + [2] for descending lengths; a length-1 caption is [2]"""
    rng = np.random.RandomState(seed)
    cap = np.zeros((len(lens), lens[0]), dtype=np.int64)
    for b, l in enumerate(lens):
        cap[b, 0] = 1
        cap[b, 1:l - 1] = rng.randint(4, V, size=max(0, l - 2))
        cap[b, l - 1] = 2
    return torch.from_numpy(cap), [int(l) for l in lens]


@functools.lru_cache(maxsize=None)
def params_of(case, cell, bf16):
    c = CASES[case]
    sd = R.init_decoder_params(c["E"], c["H"], V, c["L"], cell, seed=c["seed"], attn=dict(F=c["F"], A=c["A"]))
    sd["attn.full_att.weight"] = sd["attn.full_att.weight"] * c["scale"]
    return {k: (_bf16(v) if bf16 else v) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def problem(case, cell, bf16):
    """(params, feat (B, F, P), cap, lens): read-only"""
    c = CASES[case]
    cap, lens = captions(c["lens"], c["seed"])
    return params_of(case, cell, bf16), features(len(lens), c["F"], c["P"], c["seed"], bf16), cap, lens


@functools.lru_cache(maxsize=None)
def beam_features(case, bf16):
    """FLOOR_IMAGES images of the case's geometry; the GPU searches the first BEAM_IMAGES"""
    c = CASES[case]
    return features(FLOOR_IMAGES, c["F"], c["P"], c["seed"] + 500, bf16)


# ====================================================================================================================
# the launch arithmetic
# ====================================================================================================================

def up8(n):
    return (n + 7) // 8 * 8


def step_paths(F_, A, P, rows, bf16):
    """what attn_fwd_launch / attn_bwd_launch choose for one step of `rows` rows"""
    threads = 1024 if rows < 512 else 256
    N = 8 if bf16 else 4
    nchunk = F_ // N
    out = dict(threads=threads, N=N, nchunk=nchunk)
    for name, width in (("fwd", nchunk), ("bwd", A)):
        G = threads // width if threads >= 2 * width else 1
        per = -(-P // G)
        out[name] = dict(G=G, per=per,
                         idle=threads - G * width if G > 1 else 0,            # threads with g == G
                         empty=G - (-(-P // per)) if G > 1 else 0,            # trailing groups without a pixel
                         last_group=list(range((-(-P // per) - 1) * per, P)),   # pixels of the last group that has any
                         trips=-(-width // threads) if G == 1 else 1,         # of the G == 1 channel loop
                         lds=(G * F_ * 4 if name == "fwd" else 2 * G * A * 4) if G > 1 else 0)
    out["score_trips"] = -(-A // (64 * N))
    out["score_partial"] = A % (64 * N) != 0
    return out


def paths(case, bf16):
    c = CASES[case]
    lens = c["lens"]
    rows = R.batch_sizes(lens)
    B, n_tok = len(lens), sum(lens)
    BP = B * c["P"]
    Np = up8(max(n_tok, BP))
    return dict(rows=rows, n_tok=n_tok, BP=BP, Np=Np, pad_pixels=Np - BP, pad_tokens=Np - n_tok,
                steps=[step_paths(c["F"], c["A"], c["P"], r, bf16) for r in rows])


def beam_paths(F_, A, P, W, bf16):
    """attn_beam_fwd_launch: 1024 threads, one workgroup per image"""
    N = 8 if bf16 else 4
    nchunk = F_ // N
    G = 1024 // nchunk if 1024 >= 2 * nchunk else 1
    return dict(N=N, G=G, per=-(-P // G), kU=2 if W * N >= 56 else 4, lds=max(W * A, (G - 1) * F_) * 4)


# ====================================================================================================================
# copies of the oracle's arithmetic, with the seeded faults
# ====================================================================================================================

FORWARD_FAULTS = ("last_pixel_out", "neighbour_alpha", "score_cut", "feat_cut")


def _attention_copy(params, feat_bpf, att1, h, fault):
    """R.attention_net on a hoisted att1.  Faults: the last pixel left out of the softmax and the context; the context taken
    with the alpha of the neighbouring pixel; score channels >= 1024 ignored; feature channels >= 4096 left out of z."""
    att2 = h @ params["attn.decoder_att.weight"].t() + params["attn.decoder_att.bias"]
    e = F.leaky_relu(att1 + att2.unsqueeze(1), 0.2)
    w = params["attn.full_att.weight"]
    if fault == "score_cut":
        e, w = e[..., :1024], w[:, :1024]
    att = (e @ w.t() + params["attn.full_att.bias"]).squeeze(2)
    if fault == "last_pixel_out":
        alpha = torch.cat([torch.softmax(att[:, :-1], dim=1), torch.zeros_like(att[:, -1:])], 1)
    else:
        alpha = torch.softmax(att, dim=1)
    used = alpha.roll(1, 1) if fault == "neighbour_alpha" else alpha
    z = (feat_bpf * used.unsqueeze(2)).sum(dim=1)
    if fault == "feat_cut":
        z = torch.cat([z[:, :4096], torch.zeros_like(z[:, 4096:])], 1)
    return z, alpha


def _stored(x):
    """x as a bf16 buffer holds it, the gradient passing through unrounded"""
    return x + (R._round_bf16(x) - x).detach()


def train_copy(params, feat, cap, lens, cell, fault=None, storage=False, return_logits=False):
    """R.attn_train_loss(alpha_c = 1) with att1 = encoder_att(feat) computed once.  Returns (loss, alphas, att1 (B, P, A)), with
    `return_logits` also the packed logits (N_tok, V).
    With `storage`, every forward value that make_plan (csrc/attn.cpp) keeps in a bf16 buffer is rounded to bf16 where it is
    stored: the mean feature, h0 (c0), att1, z, both halves of x, h after every cell and c of the LSTM (feat and the weights are
    bf16-representable already).  The backward stays float64."""
    st = _stored if storage else (lambda x: x)
    B, T = cap.shape
    L = R.num_layers_of(params)
    emb = params["embeddings.weight"][cap]
    mean = st(feat.mean(dim=2))
    h = st(mean @ params["init_h.weight"].t() + params["init_h.bias"]).unsqueeze(0).repeat(L, 1, 1)
    c = None
    if cell != "gru":
        c = st(mean @ params["init_c.weight"].t() + params["init_c.bias"]).unsqueeze(0).repeat(L, 1, 1)
    feat_bpf = feat.transpose(1, 2)
    att1 = st(feat_bpf @ params["attn.encoder_att.weight"].t() + params["attn.encoder_att.bias"])
    if att1.requires_grad:
        att1.retain_grad()
    preds = feat.new_zeros(B, T, params["linear.weight"].shape[0])
    alphas = feat.new_zeros(B, T, feat.shape[2])
    for t in range(T):
        bt = sum(1 for l in lens if l > t)
        z, alpha = _attention_copy(params, feat_bpf[:bt], att1[:bt], h[-1, :bt], fault)
        ez = st(z) @ params["embed.weight"].t() + params["embed.bias"]
        inp, hs, cs = st(torch.cat([emb[:bt, t], ez], 1)), [], []
        for l in range(L):                                                  # R.rnn_step, layer by layer
            w = R._layer_w(params, l)
            if cell == "gru":
                inp = st(R.gru_cell(inp, h[l, :bt], *w))
            else:
                inp, cl = R.lstm_cell(inp, h[l, :bt], c[l, :bt], *w)
                inp = st(inp)
                cs.append(st(cl))
            hs.append(inp)
        h, c = torch.stack(hs, 0), (torch.stack(cs, 0) if cs else None)
        preds[:bt, t] = inp @ params["linear.weight"].t() + params["linear.bias"]
        alphas[:bt, t] = alpha
    logits = R.pack_rows(preds, lens)
    loss = R.ce_loss(logits, R.pack_rows(cap, lens)) + ((1.0 - alphas.sum(dim=1)) ** 2).mean()
    return (loss, alphas, att1, logits) if return_logits else (loss, alphas, att1)


@functools.lru_cache(maxsize=None)
def train_copy_grads(case, cell, fault=None, bf16=False, storage=False):
    """float64 (loss, alphas, {name: gradient}) of the copy.  The gradient faults act on the encoder_att contraction
    d W_e = sum over the B*P rows of d att1[row]^T feat[row]:
      phantom_row       one more row, a copy of row 0 (a pad column of the transposed operands that is not zero)
      last_group_datt1  the rows of the last pixel group of the 1024-thread backward are missing (its d att1 not accumulated)"""
    params, feat, cap, lens = problem(case, cell, bf16)
    po = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    fd = feat.double()
    loss, alphas, att1 = train_copy(po, fd, cap, lens, cell, fault if fault in FORWARD_FAULTS else None, storage)
    loss.backward()
    g = {k: p.grad.clone() for k, p in po.items()}
    d1, fb = att1.grad, fd.transpose(1, 2)
    if fault == "phantom_row":
        g["attn.encoder_att.weight"] += d1[0, 0][:, None] * fb[0, 0][None, :]       # the bias is a column sum of its own
    elif fault == "last_group_datt1":
        c = CASES[case]
        px = step_paths(c["F"], c["A"], c["P"], 1, bf16)["bwd"]["last_group"]
        g["attn.encoder_att.weight"] -= torch.einsum("bpa,bpf->af", d1[:, px], fb[:, px])
        g["attn.encoder_att.bias"] -= d1[:, px].sum((0, 1))
    return loss.item(), alphas.detach(), g


def beam_step_copy(params, ctx, tok, state, par_next=None, cell="gru", storage=True, slot_fault=False):
    """R.attn_beam_step_bf16_storage; with `slot_fault` slot w >= 1 of an image reads att2 of slot w - 1"""
    tok = torch.as_tensor(np.asarray(tok), dtype=torch.long)
    B, W = tok.shape
    h, c = state
    feat, att1 = ctx["feat"], ctx["att1"]
    att2 = (h[-1] @ params["attn.decoder_att.weight"].t() + params["attn.decoder_att.bias"]).view(B, W, 1, -1)
    if slot_fault:
        att2 = att2[:, [0] + list(range(W - 1))]
    e = F.leaky_relu(att1.unsqueeze(1) + att2, 0.2)
    att = (e @ params["attn.full_att.weight"].reshape(-1)) + params["attn.full_att.bias"]
    alpha = torch.softmax(att, dim=2)
    z = R._store(torch.bmm(alpha, feat).reshape(B * W, -1), storage)
    ez = R._store(z @ params["embed.weight"].t() + params["embed.bias"], storage)
    x = torch.cat([R._store(params["embeddings.weight"][tok.reshape(-1)], storage), ez], 1)
    top, h, c = R._cells_storage(params, x, h, c, cell, storage)
    logp = torch.log_softmax(top @ params["linear.weight"].t() + params["linear.bias"], 1)
    new = (h, c)
    return logp, alpha.reshape(B * W, -1), (new if par_next is None else R.beam_gather_state(new, par_next, W))


# ====================================================================================================================
# greedy decoding along given tokens, and the floors
# ====================================================================================================================

def greedy_walk(params, feat, cell, storage, dt=torch.float64, tokens=None, start_id=1):
    """The restatement of st_attn_greedy (R.attn_beam_*_bf16_storage at W = 1; `storage`: rounded to bf16 where the bf16 kernels
    store).  Step t is fed tokens[:, t - 1] (the start token at t = 0) from the walk's OWN state; without `tokens` it feeds its
    own arg-max.  Returns (logp (B, STEPS, V), alpha (B, STEPS, P), arg-max ids (B, STEPS))."""
    orc = StepOracle("attn", cell, params, feat, 1, storage, dt)
    B = feat.shape[0]
    _, state = orc.start()
    tok = torch.full((B, 1), start_id, dtype=torch.long)
    lps, als, ids = [], [], []
    for t in range(STEPS):
        logp, alpha, state = orc.step(tok, state)
        lps.append(logp); als.append(alpha); ids.append(logp.max(1)[1])
        tok = (ids[-1] if tokens is None else tokens[:, t]).view(B, 1)
    return torch.stack(lps, 1), torch.stack(als, 1), torch.stack(ids, 1)


def top_two_gap(logp):
    tv = torch.topk(logp.double(), 2, dim=-1)[0]
    return tv[..., 0] - tv[..., 1]


@functools.lru_cache(maxsize=None)
def greedy_floor(case, cell, bf16):
    """(largest |d logp| between fp32 and float64 arithmetic of the walk along the float64 walk's own tokens, the float64 walk's
    top-two gaps (B, STEPS))"""
    params, feat, _, _ = problem(case, cell, bf16)
    lp64, _, ids = greedy_walk(params, feat, cell, bf16)
    lp32, _, _ = greedy_walk(params, feat, cell, bf16, torch.float32, ids)
    return (lp32.double() - lp64).abs().max().item(), top_two_gap(lp64)


@functools.lru_cache(maxsize=None)
def greedy_gap(bf16):
    """GAP: 4 x the largest |d logp| of greedy_floor over GREEDY_CASES and both cells"""
    return 4 * max(greedy_floor(case, cell, bf16)[0] for case in GREEDY_CASES for cell in ("gru", "lstm"))


def beam_oracle(cell, params, feat, W, storage, dt=torch.float64, slot_fault=False):
    """the attention decoder's StepOracle; with `slot_fault` on beam_step_copy's faulted step"""
    fn = (lambda o, tok, state: beam_step_copy(o.p, o.ctx, tok, state, None, o.cell, o.storage, True)) if slot_fault else None
    return StepOracle("attn", cell, params, feat, W, storage, dt, fn)


@functools.lru_cache(maxsize=None)
def beam_floor(case, cell, bf16, W):
    """fp32 against float64 arithmetic of the same restatement, teacher-forced on the float64 oracle's own free-running records of
    FLOOR_IMAGES images"""
    params, feat = params_of(case, cell, bf16), beam_features(case, bf16)
    o64 = beam_oracle(cell, params, feat, W, bf16)
    return beam_distance(beam_oracle(cell, params, feat, W, bf16, torch.float32), o64, o64.free_run(BEAM_T))


def storage_distance(case, cell):
    """{tensor: (rel_l2, rel_max)} between the float64 oracle and the same oracle with bf16 rounding at make_plan's storage points
    (train_copy's `storage`), both on the bf16-representable inputs of the case: what bf16 storage alone does to each gradient"""
    _, _, g = train_copy_grads(case, cell, None, True)
    _, _, gs = train_copy_grads(case, cell, None, True, True)
    out = {}
    for k in g:
        d = gs[k] - g[k]
        out[k] = ((d.norm() / (g[k].norm() + 1e-300)).item(), (d.abs().max() / (g[k].abs().max() + 1e-300)).item())
    return out
