"""The numpy replica of the decoders' dropout mask, the cases, the float64 oracle and the seeded faults that
tests/test_gpu_dropout.py and tests/test_dropout_inputs.py share.

Mask (csrc/dropout.h): words = Philox4x32-10(counter = (column / 4, packed row, site, step), key = (seed low 32, seed high 32)),
word e belongs to column 4 * (column / 4) + e; kept iff word >= floor(p * 2^32) (float64); a kept element is
T(float32(x) * float32(1 / (1 - p))), a dropped one +0.  Sites: l = output of recurrent layer l, SITE_INPUT = the layer-0 input.

Oracle: oracle.restatement's gru_cell / lstm_cell, pack_rows and batch_sizes walked layer by layer in float64 with the replica's
masks (as float64 multipliers: float32(scale) or 0) at the three sites, autograd for the gradients; for the attention decoders
the restatement's step loop with the mask on the rows handed to `linear`.  With every p = 0 it performs the operations of
R.gru_train_loss / R.attn_train_loss in their order.  Every reference is computed once per process (lru_cache) and handed out as
is: callers do not modify it.

Bounds are those of the files that test the same quantities without dropout: tests/test_gpu_decoder.py (fp32: loss 2e-5, relative
max 2e-4; bf16: loss 2e-2, relative max 4e-2) and tests/test_gpu_attention.py (fp32: loss 3e-5, relative max 3e-4, alphas 2e-4).

Faults (what a wrong kernel or a wrong host side would compute, expressed in the oracle): tests/test_dropout_inputs.py shows that
each moves at least one compared quantity of every case by 10 x its bound, so the GPU comparison can tell them from the truth."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import restatement as R
from tests._util import load_fixture

SITE_INPUT = 255
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
U32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: 4 uint32 arrays (broadcastable), key: 2 ints -> 4 uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & U32 for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & U32, int(key[1]) & U32
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & np.uint64(U32), (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & np.uint64(U32)]
        k0, k1 = (k0 + W0) & U32, (k1 + W1) & U32
    return [x.astype(np.uint32) for x in c]


def threshold(p):
    return int(np.floor(np.float64(p) * 4294967296.0))


def scale_of(p):
    return np.float32(1.0 / (1.0 - np.float64(p)))


def words(seed, step, site, rows, cols, row0=0):
    """(rows, cols) uint32: the word of every element of a rows x cols matrix whose first row is packed row row0."""
    assert cols % 4 == 0
    seed = int(seed) & ((1 << 64) - 1)
    r = np.arange(row0, row0 + rows, dtype=np.uint64)[:, None]
    c4 = np.arange(cols // 4, dtype=np.uint64)[None, :]
    w = philox4x32_10((c4, r, np.uint64(site), np.uint64(step)), (seed & U32, seed >> 32))
    return np.stack(w, axis=-1).reshape(rows, cols)


def keep_mask(seed, step, site, rows, cols, p, row0=0):
    return words(seed, step, site, rows, cols, row0) >= np.uint32(threshold(p))


def bf16_round(x32):
    """float32 array -> the nearest bf16 (ties to even) as float32."""
    u = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + ((u >> np.uint64(16)) & np.uint64(1)) + np.uint64(0x7FFF)) & np.uint64(0xFFFF0000)
    return u.astype(np.uint32).view(np.float32)


def dropout_rows(x, p, seed, step, site, row0=0, bf16=False):
    """The replica of st_dropout_rows on a float32 numpy matrix (bf16: holding bf16 values; the result is rounded to bf16)."""
    x = np.asarray(x, dtype=np.float32)
    keep = words(seed, step, site, x.shape[0], x.shape[1], row0) >= np.uint32(threshold(p))
    y = np.where(keep, x * scale_of(p), np.float32(0.0)).astype(np.float32)
    return bf16_round(y) if bf16 else y


def multiplier(seed, step, site, rows, cols, p, row0=0, scale=True):
    """The mask as a float64 torch multiplier: float32(1 / (1 - p)) (1 with scale=False) where kept, 0 where dropped."""
    keep = words(seed, step, site, rows, cols, row0) >= np.uint32(threshold(p))
    return torch.from_numpy(np.where(keep, np.float64(scale_of(p)) if scale else 1.0, 0.0))


# ---- cases -------------------------------------------------------------------------------------------------------------
# name: (family, cell, dtype, E, H, V, L, B, (p_in, p_layer, p_out), seed)
# fp32 / bf16 launch chain: more than one 16-row tile (B = 19), B_{t+1} < B_t, in0 != H and an H that is no multiple of 16 (fp32)
P_FP32 = {"all": (0.2, 0.3, 0.5), "in": (0.2, 0.0, 0.0), "layer": (0.0, 0.3, 0.0), "out": (0.0, 0.0, 0.5)}
P_BF16 = {"all": (0.5, 0.4, 0.6), "in": (0.5, 0.0, 0.0), "layer": (0.0, 0.5, 0.0), "out": (0.0, 0.0, 0.5)}
LENS19 = [9, 9, 8, 8, 7, 7, 6, 6, 5, 5, 4, 4, 3, 3, 2, 2, 1, 1, 1]
CASES = {}
for _cell in ("gru", "lstm"):
    for _k, _p in P_FP32.items():
        CASES[f"{_cell}_fp32_{_k}"] = ("rnn", _cell, "fp32", 48, 72, 200, 3, 19, _p, 0x1234567 + len(_k))
    for _k, _p in P_BF16.items():
        CASES[f"{_cell}_bf16_{_k}"] = ("rnn", _cell, "bf16", 64, 64, 200, 3, 19, _p, 0x89ABCDEF0123 + len(_k))
CASES["gru_bf16_fused"] = ("rnn", "gru", "bf16", 512, 512, 777, 2, 9, (0.5, 0.4, 0.6), (0xFEDCBA98 << 32) | 0x76543210)   # bit 63 set
CASES["gru_bf16_fused_w_ls"] = ("rnn", "gru", "bf16", 512, 512, 777, 2, 9, (0.5, 0.4, 0.6), 77)   # + token_weight and label_smoothing
CASES["attn_gru_fp32"] = ("attn", "gru", "fp32", 32, 64, 50, 3, 4, (0.0, 0.0, 0.5), 2024)
CASES["attn_lstm_fp32"] = ("attn", "lstm", "fp32", 32, 64, 50, 3, 4, (0.0, 0.0, 0.5), 2025)
RNN_CASES = [c for c in CASES if CASES[c][0] == "rnn"]
ATTN_CASES = [c for c in CASES if CASES[c][0] == "attn"]
LABEL_SMOOTHING = {"gru_bf16_fused_w_ls": 0.3}
# (loss absolute, gradients relative to max |reference|)
BOUNDS = {("rnn", "fp32"): (2e-5, 2e-4), ("rnn", "bf16"): (2e-2, 4e-2), ("attn", "fp32"): (3e-5, 3e-4)}
ALPHAS_BOUND = 2e-4
ZERO_GRADS = ("attn.full_att.bias",)          # softmax is shift invariant: analytically zero, fp32 noise on both sides


def bounds(case):
    return BOUNDS[(CASES[case][0], CASES[case][2])]


def torch_dtype(case):
    return torch.bfloat16 if CASES[case][2] == "bf16" else torch.float32


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(params, feat, caption, lens, alpha_c) as fp32 CPU tensors, bf16-representable for the bf16 cases."""
    family, cell, dt, E, H, V, L, B, _, _ = CASES[case]
    if family == "attn":
        params, _, d = load_fixture(f"attn_{cell}_small.npz")
        return params, torch.from_numpy(d["feat"]), torch.from_numpy(d["caption"]), d["lens"].tolist(), float(d["alpha_c"])
    params = R.init_decoder_params(E, H, V, L, cell, seed=13)
    if H == 512:
        cap, lens = R.synthetic_captions(B, V, seed=5, mean=7, std=2, lo=3, hi=11)
    else:
        lens = list(LENS19)
        rng = np.random.RandomState(13)
        capn = np.zeros((B, lens[0]), dtype=np.int64)
        for b, l in enumerate(lens):
            capn[b, :l] = rng.randint(4, V, size=l)
        cap = torch.from_numpy(capn)
    feat = torch.randn(B, E, generator=torch.Generator().manual_seed(13))
    if dt == "bf16":
        params = {k: v.bfloat16().float() for k, v in params.items()}
        feat = feat.bfloat16().float()
    return params, feat, cap, lens, 0.0


@functools.lru_cache(maxsize=None)
def token_weight(case):
    """(B, T) fp32 uniform in [-1, 1] for the case that combines weights with dropout; None for the others."""
    if case not in LABEL_SMOOTHING:
        return None
    cap = inputs(case)[2]
    return torch.rand(tuple(cap.shape), generator=torch.Generator().manual_seed(31)) * 2 - 1


# ---- faults ------------------------------------------------------------------------------------------------------------
# None: the truth.  Otherwise one of:
#   "row_shift"      every mask generated one packed row off
#   "sites_rotated"  every site uses the counter of the next one in [input, 0, 1, .., L - 1]
#   "no_bwd_in" / "no_bwd_layer" / "no_bwd_out"   the backward pass forgets the mask (and scale) at that site
#   "dw_undropped"   dW_ih of the layers above the first contracts with the plain rows of the layer below
#   "no_scale"       kept elements are not scaled, forward and backward
FAULTS = ("row_shift", "sites_rotated", "no_bwd_in", "no_bwd_layer", "no_bwd_out", "dw_undropped", "no_scale")


def faults_of(case):
    """The faults that can touch the case: a site that is off has no mask to get wrong."""
    family, _, _, _, _, _, L, _, (p_in, p_layer, p_out), _ = CASES[case]
    out = ["row_shift", "sites_rotated", "no_scale"]
    if p_in:
        out.append("no_bwd_in")
    if p_layer and L > 1:
        out += ["no_bwd_layer", "dw_undropped"]
    if p_out:
        out.append("no_bwd_out")
    return out


class _Mask(torch.autograd.Function):
    """y = x * mf on the way forward, dx = dy * mb on the way back (mb is not mf only under a seeded fault)."""

    @staticmethod
    def forward(ctx, x, mf, mb):
        ctx.save_for_backward(mb)
        return x * mf

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None, None


class _InputProj(torch.autograd.Function):
    """x_read W^T, whose weight gradient contracts with x_dw (the seeded fault 'dw_undropped': x_dw is not x_read)."""

    @staticmethod
    def forward(ctx, x_read, x_dw, w):
        ctx.save_for_backward(x_dw, w)
        return x_read @ w.t()

    @staticmethod
    def backward(ctx, g):
        x_dw, w = ctx.saved_tensors
        return g @ w, None, g.t() @ x_dw


def _site_masks(case, step, ntok, fault):
    """site -> (forward multiplier, backward multiplier) as float64 (ntok, width) tensors, or None where the site is off."""
    family, _, _, E, H, _, L, _, (p_in, p_layer, p_out), seed = CASES[case]
    order = [SITE_INPUT] + list(range(L))
    row0 = 1 if fault == "row_shift" else 0
    sc = fault != "no_scale"
    out = {}
    for site in order:
        p = p_in if site == SITE_INPUT else p_out if site == L - 1 else p_layer
        if not p:
            out[site] = None
            continue
        width = (E if family == "rnn" else 2 * E) if site == SITE_INPUT else H
        used = order[(order.index(site) + 1) % len(order)] if fault == "sites_rotated" else site
        mf = multiplier(seed, step, used, ntok, width, p, row0, sc)
        kind = "in" if site == SITE_INPUT else "out" if site == L - 1 else "layer"
        out[site] = (mf, torch.ones_like(mf) if fault == f"no_bwd_{kind}" else mf)
    return out


def _drop(x, m):
    return x if m is None else _Mask.apply(x, m[0], m[1])


def _loss(logits, target, w, eps):
    if w is None and not eps:
        return R.ce_loss(logits, target)
    per_row = F.cross_entropy(logits, target, reduction="none", label_smoothing=eps)
    return ((per_row if w is None else w * per_row).sum()) / per_row.shape[0]


def rnn_loss(case, params, feat, cap, lens, step=0, fault=None, dropout=True):
    """The decoder's loss with the case's masks of `step` (dropout=False: none), on the tensors given (float64 for the oracle)."""
    _, cell, _, E, H, V, L, B, _, _ = CASES[case]
    bs = R.batch_sizes(lens)
    ntok = sum(bs)
    off = np.concatenate([[0], np.cumsum(bs)])
    masks = _site_masks(case, step, ntok, fault) if dropout else {s: None for s in [SITE_INPUT] + list(range(L))}
    emb = params["embeddings.weight"][cap]                                # rnn.py:29
    raw = torch.cat((feat.unsqueeze(1), emb), 1)                          # rnn.py:30
    plain = R.pack_rows(raw, lens)                                        # (ntok, E), time-major
    rows = _drop(plain, masks[SITE_INPUT])
    for l in range(L):
        w_ih, w_hh, b_ih, b_hh = R._layer_w(params, l)
        h = rows.new_zeros(B, H)
        c = rows.new_zeros(B, H)
        out = []
        for t, b in enumerate(bs):
            x = rows[off[t]:off[t + 1]]
            if fault == "dw_undropped" and l > 0 and masks[l - 1] is not None:
                # the cell's own x W_ih^T with an identity weight: the product (and its faulty weight gradient) is formed outside
                x, wi = _InputProj.apply(x, plain[off[t]:off[t + 1]], w_ih), torch.eye(w_ih.shape[0], dtype=x.dtype)
            else:
                wi = w_ih
            if cell == "gru":
                hn = R.gru_cell(x, h[:b], wi, w_hh, b_ih, b_hh)
            else:
                hn, cn = R.lstm_cell(x, h[:b], c[:b], wi, w_hh, b_ih, b_hh)
                c = torch.cat([cn, c[b:]], 0)
            h = torch.cat([hn, h[b:]], 0)
            out.append(hn)
        plain = torch.cat(out, 0)
        rows = _drop(plain, masks[l])
    logits = rows @ params["linear.weight"].t() + params["linear.bias"]  # rnn.py:33
    tw = token_weight(case)
    w = None if tw is None else R.pack_rows(tw.to(logits.dtype), lens)
    return _loss(logits, R.pack_rows(cap, lens), w, LABEL_SMOOTHING.get(case, 0.0)), logits, None


def attn_loss(case, params, feat, cap, lens, alpha_c, step=0, fault=None, dropout=True):
    """R.attn_forward's step loop (rnn_attn.py:63-76) with the mask on the rows handed to `linear`, then main_attn.py:126-131."""
    _, cell, _, E, H, V, L, B, _, _ = CASES[case]
    bs = R.batch_sizes(lens)
    off = np.concatenate([[0], np.cumsum(bs)])
    m = _site_masks(case, step, sum(bs), fault)[L - 1] if dropout else None
    T, P = cap.shape[1], feat.shape[2]
    emb = params["embeddings.weight"][cap]
    h, c = R._attn_init(params, feat, cell)
    feat_bpf = feat.transpose(1, 2)
    preds = feat.new_zeros(B, T, V)
    alphas = feat.new_zeros(B, T, P)
    for t in range(T):
        bt = sum(1 for l in lens if l > t)
        if bt == 0:
            break
        z, alpha = R.attention_net(params, feat_bpf[:bt], h[-1, :bt])
        ez = z @ params["embed.weight"].t() + params["embed.bias"]
        top, h, c = R.rnn_step(params, torch.cat([emb[:bt, t], ez], 1), h[:, :bt], None if c is None else c[:, :bt], cell)
        if m is not None:
            top = _Mask.apply(top, m[0][off[t]:off[t + 1]], m[1][off[t]:off[t + 1]])
        preds[:bt, t] = top @ params["linear.weight"].t() + params["linear.bias"]
        alphas[:bt, t] = alpha
    logits = R.pack_rows(preds, lens)
    loss = R.ce_loss(logits, R.pack_rows(cap, lens))
    return loss + alpha_c * ((1.0 - alphas.sum(dim=1)) ** 2).mean(), logits, alphas


@functools.lru_cache(maxsize=None)
def oracle(case, step=0, fault=None):
    """(loss, {name: gradient, 'feat': gradient}, logits, alphas) in float64 of the case at mask step `step`."""
    params, feat, cap, lens, alpha_c = inputs(case)
    po = {k: v.double().requires_grad_(True) for k, v in params.items()}
    fo = feat.double().requires_grad_(True)
    if CASES[case][0] == "attn":
        loss, logits, alphas = attn_loss(case, po, fo, cap, lens, alpha_c, step, fault)
    else:
        loss, logits, alphas = rnn_loss(case, po, fo, cap, lens, step, fault)
    loss.backward()
    grads = {k: v.grad.detach() for k, v in po.items()}
    grads["feat"] = fo.grad.detach()
    return loss.item(), grads, logits.detach(), None if alphas is None else alphas.detach()


def rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-300)).item()
