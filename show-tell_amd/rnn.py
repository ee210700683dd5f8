"""Decoder: drop-in for the reference's ``rnn.RNN`` (rnn.py:10-108) and, through the
``cell`` switch, ``LSTM/rnn_lstm.RNN`` (rnn_lstm.py:8-57).

Same constructor, same attribute names (``embeddings``, ``unit``, ``linear``) and
``state_dict`` keys, same call conventions:

    logits = rnn(cnn_feature, image_caption, caption_size)      # (N_tok, V), time-major packed rows
    ids    = rnn.sentence_index(cnn_feature, beam_size=0)       # Long(B, 25) (squeezed)
    ids, logp, lengths = rnn.sample(cnn_feature, num_samples=5, temperature=0.8, top_k=20)   # (B, S, 25) draws (st_rnn_sample)
    loss   = rnn.loss(cnn_feature, image_caption, caption_size, sequence_weight=advantage)   # sum w * nll / N_tok (reward-weighted)
    loss   = rnn.loss(cnn_feature, image_caption, caption_size, label_smoothing=0.1)         # CrossEntropyLoss(label_smoothing=0.1)
    logp   = rnn.token_logp(cnn_feature, image_caption, caption_size)                        # (B, T) log p of every given token
    rnn    = RNN(E, H, V, L, dropout=0.3, dropout_out=0.5); rnn.train() / rnn.eval()         # nn.GRU(dropout=) + Dropout before linear
    ids, replaced = rnn.scheduled_inputs(cnn_feature, image_caption, caption_size, p=0.25)    # scheduled sampling's roll-in
    loss   = rnn.loss(cnn_feature, image_caption, caption_size, input_ids=ids)                # ... or scheduled_sampling=0.25

``nn.Embedding`` / ``nn.GRU`` / ``nn.Linear`` objects are parameter containers only; all
arithmetic runs in libshowtell_hip (st_rnn_forward / st_rnn_backward / st_rnn_greedy /
st_cross_entropy).  ``loss()`` is the fused route (vocabulary projection + cross entropy
without handing fp32 logits to torch) used by the training driver and bench.py.
A training call is one st_rnn_forward, one loss call (st_rnn_fused_loss, or st_cross_entropy
on st_rnn_forward's logits), one dlogits call and one st_rnn_backward, whatever the keywords:
dropout travels as an st_dropout, ``input_ids`` as a pointer, and weights, per-row outputs and
label smoothing as one st_loss_terms (``loss_terms``); NULL / None for each is the plain call.

Gradients: the backward kernels accumulate straight into ``param.grad`` (fp32), so after
``loss.backward()`` the optimizer sees exactly what torch autograd would have produced.
"""
import ctypes as C
import os

import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import ST_CELL_GRU, ST_CELL_LSTM, ST_F32, LossTerms, RnnGrads, RnnParams, check, dtype_code, lib, ref
from ._lib import ptr as _cp, stream as _stream  # noqa: F401  (tests and tools import these names from here)
from .dropout import DropoutState
from ._weights import FollowsMoves, grad_buffer, working_copy  # noqa: F401  (rnn.working_copy stays importable)
from .seq import plan_for

CAP_MAX = 25  # rnn.py:39

_LAYER_NAMES = [tuple(f"{n}_l{l}" for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")) for l in range(_lib.ST_MAX_LAYERS)]


def up8(v):
    return (v + 7) // 8 * 8


def check_sample_args(vocab_size, batch, num_samples, temperature, top_k, max_length, uniforms, top_p=1.0):
    """Argument errors of ``sample`` (both decoders), raised before anything touches the device."""
    if isinstance(top_p, bool) or not isinstance(top_p, (int, float)) or not 0 < top_p <= 1:        # NaN fails both comparisons
        raise ValueError(f"top_p must be in (0, 1], 1 switching the nucleus off (got {top_p!r})")
    if not temperature > 0:
        raise ValueError(f"temperature must be > 0 (got {temperature})")
    if int(top_k) != top_k or not 0 <= top_k <= min(32, vocab_size):
        raise ValueError(f"top_k must be 0 (the whole vocabulary) or 1..{min(32, vocab_size)} (got {top_k})")
    if int(num_samples) != num_samples or num_samples < 1:
        raise ValueError(f"num_samples must be >= 1 (got {num_samples})")
    if int(max_length) != max_length or max_length < 1:
        raise ValueError(f"max_length must be >= 1 (got {max_length})")
    if uniforms is not None:
        want = (batch, int(num_samples), int(max_length))
        if not torch.is_tensor(uniforms) or tuple(uniforms.shape) != want or uniforms.dtype != torch.float32:
            raise ValueError(f"uniforms must be a float32 tensor of shape {want} (images, samples, steps)")


def sample_uniforms(uniforms, shape, device, generator):
    """The (B, S, T) fp32 uniforms of a ``sample`` call on `device`: the caller's, or torch.rand from `generator`."""
    if uniforms is not None:
        return uniforms.detach().to(device).contiguous()
    if generator is not None and generator.device.type != device.type:
        return torch.rand(shape, generator=generator, dtype=torch.float32).to(device)
    return torch.rand(shape, device=device, generator=generator, dtype=torch.float32)


def sample_lengths(ids, end_id):
    """Tokens up to and including the first <end> of every row; the row's width if it never drew <end>."""
    before = ((ids == end_id).cumsum(-1) == 0).sum(-1)
    return (before + 1).clamp(max=ids.shape[-1])


def check_weight_args(batch, width, sequence_weight, token_weight):
    """Argument errors of the loss weights (both decoders), raised before anything touches the device: `sequence_weight` is a
    (batch,) and `token_weight` a (batch, width) floating-point tensor, width that of the caption tensor."""
    for name, w, want in (("sequence_weight", sequence_weight, (batch,)), ("token_weight", token_weight, (batch, width))):
        if w is None:
            continue
        if not torch.is_tensor(w) or not w.dtype.is_floating_point or tuple(w.shape) != want:
            raise ValueError(f"{name} must be a floating-point tensor of shape {want}"
                             + (f" (got {w.dtype}, {tuple(w.shape)})" if torch.is_tensor(w) else f" (got {type(w).__name__})"))


def check_label_smoothing(label_smoothing):
    """Argument error of `label_smoothing` (both decoders and the Trainer), raised before anything touches the device: a number in
    [0, 1), as torch's CrossEntropyLoss takes it (1.0 and NaN are refused).  Returns it as a float."""
    try:
        eps = float(label_smoothing)
    except (TypeError, ValueError):
        raise ValueError(f"label_smoothing must be a number in [0, 1) (got {label_smoothing!r})") from None
    if not 0.0 <= eps < 1.0:
        raise ValueError(f"label_smoothing must be in [0, 1) (got {label_smoothing!r})")
    return eps


def check_caption_args(caption, lens):
    """Argument errors of a (caption, caption_size) pair, before anything touches the device."""
    if not torch.is_tensor(caption) or caption.dim() != 2 or caption.dtype != torch.int64:
        raise ValueError("image_caption must be a (B, T) LongTensor")
    if len(lens) != caption.shape[0] or max(int(l) for l in lens) > caption.shape[1]:
        raise ValueError(f"caption_size must hold {caption.shape[0]} lengths of at most {caption.shape[1]}")


def check_probability(p, name="p"):
    """Argument error of a scheduled-sampling rate (both decoders and the Trainer): a number in [0, 1] (NaN is refused).  Returns it
    as a float."""
    try:
        q = float(p)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number in [0, 1] (got {p!r})") from None
    if not 0.0 <= q <= 1.0:
        raise ValueError(f"{name} must be in [0, 1] (got {p!r})")
    return q


def check_scheduled_args(vocab_size, feat, caption, lens, p, temperature, top_k, uniforms):
    """Argument errors of ``scheduled_inputs`` (both decoders), raised before anything touches the device.  Returns p as a float."""
    check_caption_args(caption, lens)
    if min(int(l) for l in lens) < 1:
        raise ValueError("caption_size must hold lengths of at least 1")
    if feat.shape[0] != caption.shape[0]:
        raise ValueError(f"cnn_feature holds {feat.shape[0]} images, image_caption {caption.shape[0]} captions")
    q = check_probability(p)
    if not temperature > 0:
        raise ValueError(f"temperature must be > 0 (got {temperature})")
    if int(top_k) != top_k or not 0 <= top_k <= min(32, vocab_size):
        raise ValueError(f"top_k must be 0 (the whole vocabulary) or 1..{min(32, vocab_size)} (got {top_k})")
    if uniforms is not None:
        want = (2,) + tuple(caption.shape)
        if not torch.is_tensor(uniforms) or tuple(uniforms.shape) != want or uniforms.dtype != torch.float32:
            raise ValueError(f"uniforms must be a float32 tensor of shape {want} (coins and draws; images; slots)")
        if uniforms.device != caption.device:
            raise ValueError(f"uniforms must be on the captions' device {caption.device} (got {uniforms.device})")
    return q


def check_input_ids(input_ids, caption, vocab_size):
    """Argument errors of `input_ids` (both decoders), raised before any kernel runs: an int64 tensor of the caption tensor's shape
    and device with every id in [0, vocab_size).  The range check reads the tensor (one synchronisation when it lives on the
    device); ``loss(.., scheduled_sampling=p)`` feeds the roll-in's own ids and skips it."""
    if not torch.is_tensor(caption) or caption.dim() != 2 or caption.dtype != torch.int64:
        raise ValueError("image_caption must be a (B, T) LongTensor")
    if not torch.is_tensor(input_ids) or input_ids.dtype != torch.int64 or tuple(input_ids.shape) != tuple(caption.shape):
        raise ValueError(f"input_ids must be a LongTensor of the captions' shape {tuple(caption.shape)}")
    if input_ids.device != caption.device:
        raise ValueError(f"input_ids must be on the captions' device {caption.device} (got {input_ids.device})")
    if input_ids.numel() and not bool(((input_ids >= 0) & (input_ids < vocab_size)).all()):
        raise ValueError(f"input_ids must lie in [0, {vocab_size})")


def scheduled_loss_inputs(module, feat, caption, lens, input_ids, scheduled_sampling, temperature, top_k, generator, uniforms):
    """The `input_ids` a ``loss`` call trains on: the caller's (checked), the roll-in's for scheduled_sampling = p > 0, or None
    (p = 0: no roll-in, the plain call).  Argument errors are raised before anything touches the device."""
    p = check_probability(scheduled_sampling, "scheduled_sampling")
    if input_ids is not None:
        if p:
            raise ValueError("input_ids and scheduled_sampling are exclusive")
        check_input_ids(input_ids, caption, module.vocab_size)
        return input_ids
    if not p:
        return None
    return module.scheduled_inputs(feat, caption, lens, p, temperature, top_k, generator, uniforms)[0]


def pack_row_weights(plan, sequence_weight, token_weight, device):
    """The weight of every packed row (t, b) as the kernels read it: sequence_weight[b] * token_weight[b, t], fp32 (ntok,) on
    `device`, gathered there with the plan's row map; None when neither is given.  Constants of the loss: detached."""
    if sequence_weight is None and token_weight is None:
        return None
    rb, rt = plan.row_index(device)
    w = None
    if sequence_weight is not None:
        w = sequence_weight.detach().to(device=device, dtype=torch.float32)[rb]
    if token_weight is not None:
        tw = token_weight.detach().to(device=device, dtype=torch.float32)[rb, rt]
        w = tw if w is None else w * tw
    return w.contiguous()


def unpack_rows(plan, rows, width, device):
    """(B, width) from packed rows: out[b, t] = rows[row(t, b)], 0 past each length."""
    rb, rt = plan.row_index(device)
    out = torch.zeros(plan.B, width, device=device, dtype=rows.dtype)
    out[rb, rt] = rows
    return out


def loss_terms(roww=None, nll=None, eps=0.0):
    """The st_loss_terms of one loss call: `roww` (n,) the rows' weights, `nll` (n,) receives the rows' unweighted, unsmoothed
    terms, eps > 0 label smoothing (the label-smoothing kernels; eps = 0 the ones without the term).  It holds addresses only:
    the caller keeps the tensors alive as long as it uses the descriptor."""
    t = LossTerms()
    t.row_weight = None if roww is None else roww.data_ptr()
    t.nll_out = None if nll is None else nll.data_ptr()
    t.smoothing, t.label_smoothing = (1, eps) if eps else (0, 0.0)
    return t


def ce_loss(logits, dt, targets, n, V, Vp, loss, terms):
    """loss += the cross entropy of the (n, Vp) logits rows (V valid columns) against `targets` with the terms of ``loss_terms``
    (`loss` may be None when the terms ask for the rows' own)."""
    check(lib().st_cross_entropy(_cp(logits), dtype_code(dt), _cp(targets), n, V, Vp, ref(terms), _cp(loss), None, 0, Vp, 1.0, None,
                                 _stream()), "st_cross_entropy")


def ce_loss_backward(logits, dt, targets, n, V, Vp, gout, terms):
    """The saved logits of ce_loss, overwritten in place by (softmax - (1 - eps) * onehot - eps / V) * dLoss / N_tok (row r times
    its weight), `terms` those of the forward call.  Returns (dlogits, dLoss as the fp32 device scalar the kernel read)."""
    gsc = gout.detach().float().contiguous()
    dtc = dtype_code(dt)
    check(lib().st_cross_entropy(_cp(logits), dtc, _cp(targets), n, V, Vp, ref(terms), None, _cp(logits), dtc, Vp, 1.0, _cp(gsc),
                                 _stream()), "st_cross_entropy(bwd)")
    return logits, gsc


def logits_grad(gout, dt, n, V, Vp, alloc):
    """mode 'logits' backward: the caller's (n, V) gradient as the (n, Vp) `dt` rows the backward GEMMs read (st_cast2d);
    `alloc` (torch.zeros / torch.empty) makes them."""
    g = gout if gout.dtype == torch.float32 else gout.float()
    if g.stride(1) != 1:
        g = g.contiguous()
    dlog = alloc(n, Vp, device=g.device, dtype=dt)
    check(lib().st_cast2d(_cp(g), _cp(dlog), ST_F32, dtype_code(dt), n, V, g.stride(0), Vp, _stream()), "st_cast2d")
    return dlog


class _DecoderFn(torch.autograd.Function):
    """mode 'logits': returns fp32 logits rows; mode 'loss': returns the mean cross entropy, every row's term times
    sequence_weight[b] * token_weight[b, t] where given and smoothed by `eps` where that is not 0; mode 'nll': returns the packed
    rows' -log p(target) (no gradient)."""

    @staticmethod
    def forward(ctx, feat, _anchor, module, caption, lens, mode, need_grad, sequence_weight, token_weight, eps=0.0, input_ids=None):
        m = module
        dev = feat.device
        if not feat.is_cuda or not m.linear.weight.is_cuda:
            raise _lib.ShowTellHipError("the decoder and its inputs must live on a HIP device (no CPU fallback in the MI355X build)")
        plan = plan_for(lens, dev)
        caption = caption.contiguous()
        seq = plan.c_struct(caption)
        prm, keep = m._c_params()
        dt = m.compute_dtype
        featd = m._feature(feat)
        roww = pack_row_weights(plan, sequence_weight, token_weight, dev)
        nbytes = lib().st_rnn_workspace_bytes(C.byref(prm), C.byref(seq))
        ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        V, Vp, n = m.vocab_size, lib().st_rnn_vocab_ld(m.vocab_size), plan.ntok
        targets = torch.empty(n, device=dev, dtype=torch.long)
        # mode 'loss' in bf16: the vocabulary projection and the cross entropy run tile by tile without a logits tensor (csrc/vocab_ce.hip);
        # ST_FUSED_CE=0 keeps st_rnn_forward's logits + st_cross_entropy
        fused = mode != "logits" and os.environ.get("ST_FUSED_CE", "1") != "0" and bool(lib().st_rnn_fused_loss_supported(C.byref(prm)))
        ldt = dt if mode == "loss" else torch.float32
        logits = None if fused else torch.empty(n, Vp, device=dev, dtype=ldt)
        # dropout: forward() and loss() of a module in train() with a site on; token_logp ('nll') scores the deterministic model.
        # The call's (seed, step) stay in ctx: the backward pass regenerates the same masks
        took = None if mode == "nll" else m._dropout.take(m.training)
        drop = dbuf = None
        if took is not None:
            drop, dbuf = m._dropout.desc(took, lib().st_rnn_dropout_bytes(C.byref(prm), C.byref(seq)), dev)
        # input_ids (scheduled sampling): the rows embed them, the targets stay the caption's; None is the call it was
        ids = None if input_ids is None else input_ids.detach().contiguous()
        check(lib().st_rnn_forward(C.byref(prm), C.byref(seq), _cp(featd), _cp(ws), nbytes, _cp(logits), dtype_code(ldt), Vp, _cp(targets),
                                   int(need_grad), ref(drop), _cp(ids), _stream()), "st_rnn_forward")
        ctx.drop, ctx.dbuf, ctx.ids = drop, dbuf, ids
        ctx.m, ctx.plan, ctx.caption, ctx.ws, ctx.mode, ctx.keep = m, plan, caption, ws, mode, keep
        ctx.feat_dtype = feat.dtype
        if mode == "logits":
            return logits[:, :V]
        loss = torch.zeros((), device=dev, dtype=torch.float32) if mode == "loss" else None
        nll = torch.empty(n, device=dev, dtype=torch.float32) if mode == "nll" else None
        terms = loss_terms(roww, nll, eps)
        ctx.fused, ctx.roww, ctx.terms = fused, roww, terms
        if fused:
            sb = lib().st_rnn_fused_loss_bytes(C.byref(prm), C.byref(seq))
            scratch = torch.empty(sb // 4, device=dev, dtype=torch.float32)
            if eps:         # label smoothing: the tile sums of the rows' logits live in a buffer of this call only
                tb = lib().st_rnn_fused_loss_ls_bytes(C.byref(prm), C.byref(seq))
                tsum = torch.empty(tb // 4, device=dev, dtype=torch.float32)
                terms.tile_sums, terms.tile_sums_bytes = tsum.data_ptr(), tb
            check(lib().st_rnn_fused_loss(C.byref(prm), C.byref(seq), _cp(ws), nbytes, _cp(targets), _cp(scratch), sb, ref(terms), _cp(loss),
                                          ref(drop), _stream()), "st_rnn_fused_loss")
            terms.tile_sums, terms.tile_sums_bytes = None, 0      # dead after the call, and st_rnn_fused_dlogits does not read them
            ctx.logits, ctx.targets, ctx.scratch = None, targets, scratch
        else:
            ce_loss(logits, ldt, targets, n, V, Vp, loss, terms)
            ctx.logits, ctx.targets = logits, targets
        if mode == "nll":
            ctx.mark_non_differentiable(nll)
            return nll
        return loss

    @staticmethod
    def backward(ctx, gout):
        m, plan = ctx.m, ctx.plan
        dev = gout.device
        dt = m.compute_dtype
        V, Vp, n = m.vocab_size, lib().st_rnn_vocab_ld(m.vocab_size), plan.ntok
        prm, keep = m._c_params()
        seq = plan.c_struct(ctx.caption)
        if ctx.mode == "logits":
            dlog = logits_grad(gout, dt, n, V, Vp, torch.zeros)   # pad columns feed the backward GEMM as K: must be zero
        elif ctx.mode != "loss":
            raise _lib.ShowTellHipError("token_logp has no gradient")
        elif ctx.fused:
            gsc = gout.detach().float().contiguous()
            dlog = torch.empty(n, Vp, device=dev, dtype=dt)
            check(lib().st_rnn_fused_dlogits(C.byref(prm), C.byref(seq), _cp(ctx.ws), ctx.ws.numel(), _cp(ctx.targets), _cp(ctx.scratch),
                                             _cp(gsc), ref(ctx.terms), _cp(dlog), Vp, ref(ctx.drop), _stream()), "st_rnn_fused_dlogits")
        else:
            dlog, gsc = ce_loss_backward(ctx.logits, dt, ctx.targets, n, V, Vp, gout, ctx.terms)
        grads, keep2 = m._c_grads()
        dfeat = torch.empty(plan.B, m.embed_dim, device=dev, dtype=torch.float32)
        check(lib().st_rnn_backward(C.byref(prm), C.byref(grads), C.byref(seq), _cp(dlog), Vp, _cp(ctx.ws), ctx.ws.numel(), _cp(dfeat),
                                    ref(ctx.drop), _cp(ctx.ids), _stream()), "st_rnn_backward")
        ctx.ws = ctx.dbuf = None
        return dfeat.to(ctx.feat_dtype), None, None, None, None, None, None, None, None, None, None


class Decoder(FollowsMoves, nn.Module):
    """What RNN and RNN_Attn share: the recurrent stack's part of the C descriptors and the set-up of ``sample``.
    A subclass has ``embeddings``, ``unit``, ``linear``, ``embed_dim``, ``hidden``, ``vocab_size``, ``num_layers`` and
    ``compute_dtype``."""

    cell = "gru"

    def seed_dropout(self, seed):
        """Set the 64-bit seed of this module's dropout masks and zero its step counter (the default seed is
        torch.initial_seed(), taken at construction).  The mask of a call is a pure function of (seed, step, site, packed row,
        column), so two modules with equal seeds and step counts drop the same elements; data-parallel replicas want different
        seeds (the Trainer seeds rank r with seed + r).  The state is two host integers and is NOT part of ``state_dict``: a
        run resumed from a checkpoint starts its masks over unless the caller seeds it."""
        self._dropout.reseed(seed)

    @property
    def dropout_seed(self):
        """The 64-bit seed of this module's dropout masks (``seed_dropout`` sets it)."""
        return self._dropout.seed

    def _layer_params(self):
        u = self.unit
        return [(getattr(u, wi), getattr(u, wh), getattr(u, bi), getattr(u, bh)) for wi, wh, bi, bh in _LAYER_NAMES[:self.num_layers]]

    def _rnn_params(self, r, in0, keep):
        """Fill the st_rnn_params `r` (layer 0 reads `in0` inputs); the working copies it points at go to `keep`.  Returns the
        function that did that for one parameter (for the weights a subclass adds)."""
        dt = self.compute_dtype

        def wc(prm):
            t = working_copy(prm, dt); keep.append(t); return t.data_ptr()
        r.cell = ST_CELL_GRU if self.cell == "gru" else ST_CELL_LSTM
        r.dtype = dtype_code(dt)
        r.L, r.in0, r.H, r.V, r.E = self.num_layers, in0, self.hidden, self.vocab_size, self.embed_dim
        r.emb = wc(self.embeddings.weight)
        for l, (wi, wh, bi, bh) in enumerate(self._layer_params()):
            r.w_ih[l], r.w_hh[l], r.b_ih[l], r.b_hh[l] = wc(wi), wc(wh), bi.data.data_ptr(), bh.data.data_ptr()
        r.w_lin, r.b_lin = wc(self.linear.weight), self.linear.bias.data.data_ptr()
        return wc

    def _rnn_grads(self, g, keep):
        """The same for the st_rnn_grads `g` and the fp32 gradient buffers (created on first use)."""
        def gb(prm):
            t = grad_buffer(prm); keep.append(t); return t.data_ptr()
        g.emb = gb(self.embeddings.weight)
        for l, (wi, wh, bi, bh) in enumerate(self._layer_params()):
            g.w_ih[l], g.w_hh[l], g.b_ih[l], g.b_hh[l] = gb(wi), gb(wh), gb(bi), gb(bh)
        g.w_lin, g.b_lin = gb(self.linear.weight), gb(self.linear.bias)
        return gb

    def _feature(self, cnn_feature):
        """The (B, E) image features as the recurrent kernels read them: detached, contiguous, in the compute dtype."""
        f = cnn_feature.detach().contiguous()
        return f if f.dtype == self.compute_dtype else ops.cast(f.float(), self.compute_dtype)

    def _sample_shape(self, cnn_feature, num_samples, temperature, top_k, max_length, uniforms, top_p=1.0):
        """(B, S, T) of a ``sample`` call, its arguments checked before anything touches the device."""
        B = cnn_feature.shape[0]
        check_sample_args(self.vocab_size, B, num_samples, temperature, top_k, max_length, uniforms, top_p)
        return B, int(num_samples), int(max_length)

    def scheduled_inputs(self, cnn_feature, image_caption, caption_size, p, temperature=1.0, top_k=0, generator=None, uniforms=None):
        """Scheduled sampling's roll-in (Bengio et al., 2015): a copy of `image_caption` in which some slots hold the model's own
        prediction, for ``forward / loss / token_logp(.., input_ids=)``.  Returns (input_ids (B, T) int64, replaced (B, T) bool).

        A slot is replaced iff the packed forward reads it (the step it feeds is < caption_size[b]) and coin[b, j] < p -- strict,
        so p = 0 replaces nothing and p = 1 every valid slot; every other slot keeps the caption's value.  RNN (GRU, LSTM): slot j
        feeds step j + 1 and takes a token drawn from step j's logits.  RNN_Attn: slot j feeds step j and, for j >= 1, takes a token
        drawn from step j - 1's logits; slot 0 (<start>) is never replaced.  The draw is that of ``sample`` (`temperature`,
        `top_k` <= 32, top_k = 1 the arg-max) on draw_u[b, j], from logits conditioned on the mixed prefix so far: true sequential
        scheduled sampling in one call (st_rnn_sched_inputs / st_attn_sched_inputs), no host round trip per token.  The randomness
        is `uniforms` (2, B, T) fp32 in [0, 1) on the device, [0] the coins and [1] the draws, or torch.rand from `generator`.

        No gradient flows through the choice (the call runs under no_grad) and the targets stay the caption.  The roll-in never
        applies dropout, as ``sample`` does not: it runs the deterministic model, train() or not; the training pass that follows
        applies dropout as usual."""
        q = check_scheduled_args(self.vocab_size, cnn_feature, image_caption, caption_size, p, temperature, top_k, uniforms)
        if not cnn_feature.is_cuda or not image_caption.is_cuda:
            raise _lib.ShowTellHipError("cnn_feature and image_caption must be on the HIP device (no CPU fallback)")
        with torch.no_grad():
            dev = cnn_feature.device
            cap = image_caption.contiguous()
            B, T = cap.shape
            u = sample_uniforms(uniforms, (2, B, T), dev, generator)
            lens = torch.tensor([int(l) for l in caption_size], dtype=torch.int32).to(dev, non_blocking=True)
            ids = torch.empty_like(cap)
            replaced = torch.empty(B, T, device=dev, dtype=torch.uint8)
            self._sched_inputs(cnn_feature, cap, lens, max(int(l) for l in caption_size), u, q, 1.0 / float(temperature), int(top_k), ids,
                               replaced)
            return ids, replaced.bool()

    @staticmethod
    def _sample_buffers(feat, B, S, T, uniforms, generator):
        """`feat` repeated for the S draws of every image (row b * S + s), n = B * S, and the per-row buffers of a ``sample``
        call: the uniforms (n * T), ids and logp (n, T)."""
        if S > 1:
            feat = feat.repeat_interleave(S, 0)
        n, dev = B * S, feat.device
        u = sample_uniforms(uniforms, (B, S, T), dev, generator)
        return feat, n, u, torch.empty(n, T, device=dev, dtype=torch.long), torch.empty(n, T, device=dev, dtype=torch.float32)


class RNN(Decoder):

    def __init__(self, embed_dim, num_hidden_units, vocab_size, num_layers, dtype=torch.float32, dropout=0.0, dropout_in=0.0,
                 dropout_out=0.0):
        '''
        Args (as the reference, rnn.py:12-19):
            embed_dim (int) : Embedding dimension between CNN and RNN
            num_hidden_units (int) : Number of hidden units
            vocab_size (int) : Size of the vocabulary
            num_layers (int) : # of layers
            dtype : kernel storage type (float32 = parity mode, bfloat16 = performance mode)
            dropout : as nn.GRU(dropout=) / nn.LSTM(dropout=): on the output of every recurrent layer but the last (warns with
                num_layers == 1, as torch does)
            dropout_in : on the layer-0 input rows [feature ; embeddings]
            dropout_out : nn.Dropout in front of `linear`
        Dropout (each p in [0, 1)) is active only while ``self.training`` and only in ``forward()`` and ``loss()`` (with every
        combination of weights and label smoothing, on the fused route and on the launch chain).  ``token_logp``,
        ``sentence_index``, ``beam_search`` and ``sample`` always run the deterministic model.  With every p = 0, or in
        ``eval()``, each call is the launch sequence it was.  Each training-mode call consumes one step of the module's mask
        counter (``seed_dropout``); its backward regenerates the same masks.  ``state_dict`` keys stay the reference's.
        '''
        super(RNN, self).__init__()
        self._dropout = DropoutState(dropout_in, dropout, dropout_out, num_layers)
        if num_layers > _lib.ST_MAX_LAYERS:
            raise ValueError(f"num_layers={num_layers} exceeds the kernel limit of {_lib.ST_MAX_LAYERS}")
        self.embeddings = nn.Embedding(vocab_size, embed_dim)
        unit_cls = nn.GRU if self.cell == "gru" else nn.LSTM
        self.unit = unit_cls(embed_dim, num_hidden_units, num_layers, batch_first=True)
        self.linear = nn.Linear(num_hidden_units, vocab_size)
        self.embed_dim, self.hidden, self.vocab_size, self.num_layers = embed_dim, num_hidden_units, vocab_size, num_layers
        self.compute_dtype = dtype

    # ---- C descriptors ---------------------------------------------------------------
    def _c_params(self):
        if not self.linear.weight.is_cuda:
            raise _lib.ShowTellHipError("the decoder must live on a HIP device (no CPU fallback in the MI355X build)")
        p, keep = RnnParams(), []
        self._rnn_params(p, self.embed_dim, keep)
        return p, keep

    def _c_grads(self):
        g, keep = RnnGrads(), []
        self._rnn_grads(g, keep)
        return g, keep

    # ---- reference surface -------------------------------------------------------------
    def _sched_inputs(self, cnn_feature, cap, lens, max_len, u, p, inv_t, top_k, ids, replaced):
        prm, keep = self._c_params()
        feat = self._feature(cnn_feature)
        B, T = cap.shape
        nbytes = lib().st_rnn_sched_inputs_workspace_bytes(C.byref(prm), B)
        ws = torch.empty(nbytes, device=feat.device, dtype=torch.uint8)
        check(lib().st_rnn_sched_inputs(C.byref(prm), _cp(feat), B, _cp(cap), T, _cp(lens), max_len, _cp(u[0]), _cp(u[1]), p, inv_t, top_k,
                                        _cp(ws), nbytes, _cp(ids), _cp(replaced), None, None, _stream()), "st_rnn_sched_inputs")

    def forward(self, cnn_feature, image_caption, caption_size, input_ids=None):
        """rnn.py:27-35: teacher-forced logits over the packed sequence, (N_tok, V) fp32.  In train() with a dropout site on, one
        step of the masks is applied (see __init__).  `input_ids` (B, T) int64 (``scheduled_inputs``): the tokens the steps
        t >= 1 embed, input_ids[b, t - 1], in place of the caption's; None is the call it was."""
        if input_ids is None:
            return _DecoderFn.apply(cnn_feature, self.linear.bias, self, image_caption, caption_size, "logits", torch.is_grad_enabled(), None, None)
        check_input_ids(input_ids, image_caption, self.vocab_size)
        return _DecoderFn.apply(cnn_feature, self.linear.bias, self, image_caption, caption_size, "logits", torch.is_grad_enabled(), None, None,
                                0.0, input_ids)

    def loss(self, cnn_feature, image_caption, caption_size, sequence_weight=None, token_weight=None, label_smoothing=0.0, input_ids=None,
             scheduled_sampling=0.0, ss_temperature=1.0, ss_top_k=0, ss_generator=None, ss_uniforms=None):
        """main.py:145-149 fused: CrossEntropyLoss()(rnn(feat, cap, lens), packed(cap)) as one scalar.

        With `sequence_weight` (B,) and / or `token_weight` (B, T) (float tensors, signed, T the caption tensor's width; both:
        their product) the scalar is sum_{b,t} w[b, t] * nll[b, t] / N_tok -- reward-weighted training (REINFORCE, self-critical
        sequence training).  The divisor stays N_tok, so weights of one give the plain loss; the weights are constants (no
        gradient flows into them) and apply inside the loss kernels: no logits tensor appears on the fused route.

        `label_smoothing` = eps in [0, 1) is CrossEntropyLoss(label_smoothing=eps): every row's term becomes
        (1 - eps) * nll + eps * (logsumexp(x) - mean(x)), times its weight where weights are given (the divisor stays N_tok).  The
        rows' mean logit is formed inside the loss kernels too; with eps = 0 the call is the one it was.

        In train() with a dropout site on (see __init__) the loss is that of one draw of the masks; eval() is deterministic.

        `input_ids` (B, T) int64: the tokens the steps t >= 1 embed in place of the caption's (``scheduled_inputs``); the targets
        stay the caption and the embedding gradient goes to the tokens that were fed.  It combines with weights, label smoothing
        and dropout; None is the call it was.  `scheduled_sampling` = p in [0, 1] is the two-step convenience:
        ``scheduled_inputs(.., p, ss_temperature, ss_top_k, ss_generator, ss_uniforms)`` and then this loss on its ids; p = 0 runs
        no roll-in at all.  The roll-in runs the deterministic model (no dropout); this pass applies dropout as usual."""
        eps = check_label_smoothing(label_smoothing)
        input_ids = scheduled_loss_inputs(self, cnn_feature, image_caption, caption_size, input_ids, scheduled_sampling, ss_temperature,
                                          ss_top_k, ss_generator, ss_uniforms)
        if sequence_weight is None and token_weight is None and not eps and input_ids is None:
            return _DecoderFn.apply(cnn_feature, self.linear.bias, self, image_caption, caption_size, "loss", torch.is_grad_enabled(),
                                    None, None)
        check_caption_args(image_caption, caption_size)
        check_weight_args(image_caption.shape[0], image_caption.shape[1], sequence_weight, token_weight)
        return _DecoderFn.apply(cnn_feature, self.linear.bias, self, image_caption, caption_size, "loss", torch.is_grad_enabled(),
                                sequence_weight, token_weight, eps, input_ids)

    def token_logp(self, cnn_feature, image_caption, caption_size, input_ids=None):
        """log p(image_caption[b, t] | image b, image_caption[b, :t]) for every token of the given captions: (B, T) fp32, T the
        caption tensor's width, 0 past caption_size[b].  No gradient, and never any dropout (train() or not: it scores the model).  -token_logp.sum() / N_tok is loss(); with the output of
        ``sample`` as captions it scores what that call's `logp` scored (at temperature 1, top_k 0; the two passes round differently).  On the fused route (bf16,
        H = 512) the vocabulary projection runs tile by tile: there is no logits tensor.  `input_ids`: as in ``forward``."""
        check_caption_args(image_caption, caption_size)
        if input_ids is not None:
            check_input_ids(input_ids, image_caption, self.vocab_size)
        with torch.no_grad():
            nll = _DecoderFn.apply(cnn_feature, self.linear.bias, self, image_caption, caption_size, "nll", False, None, None, 0.0, input_ids)
            return unpack_rows(plan_for(caption_size, nll.device), -nll, image_caption.shape[1], nll.device)

    def beam_search(self, cnn_feature, beam_width=4, num_hypotheses=1, max_length=50, start_id=1, end_id=2, min_length=0,
                    no_repeat_ngram_size=0, suppress_tokens=None, length_penalty=0.0, num_beam_groups=1, diversity_penalty=0.0):
        """beam_search.py:45-97 over the whole batch (BASELINE config 5: beam_width=5, max_length=25).  The last four arguments
        constrain the search (beam.beam_search): at least `min_length` words before <end>, no n-gram of that size twice in a
        caption, ids that never appear, and hypotheses ranked by cost / n**length_penalty.  `num_beam_groups` = G > 1 is diverse
        beam search (beam.beam_search): G groups of beam_width / G slots, `diversity_penalty` per earlier group's slot that took the
        same word at this step; the result is then, per image, a list of G lists of hypotheses."""
        from .beam import beam_search
        return beam_search(self, cnn_feature, beam_width, num_hypotheses, max_length, start_id, end_id, min_length=min_length,
                           no_repeat_ngram_size=no_repeat_ngram_size, suppress_tokens=suppress_tokens, length_penalty=length_penalty,
                           num_beam_groups=num_beam_groups, diversity_penalty=diversity_penalty)

    def sample(self, cnn_feature, num_samples=1, temperature=1.0, top_k=0, max_length=CAP_MAX, end_id=2, generator=None,
               uniforms=None, top_p=1.0):
        """The loop of rnn.py:37-58 with a draw in place of max(1)[1]: `num_samples` captions per image from
        softmax(logits / temperature), restricted to the `top_k` most likely words when top_k > 0 (at most 32).  One
        st_rnn_sample call for all B * num_samples rows (row b * S + s), no host round trip per token.  The randomness is
        `uniforms` (B, S, T) fp32 in [0, 1) on the device, one per row and step, or torch.rand from `generator`.

        `top_p` < 1 adds nucleus sampling (Holtzman et al., 2020).  The three filters apply in the order temperature, top_k,
        top_p: with z = logits / temperature, and restricted to the top_k set first when top_k > 0 (the probabilities below
        are renormalised over it), order the words by z descending, the lowest index first among equal values; a word is kept
        iff the probability mass strictly before it in that order is below top_p.  The first word is always kept, words of
        probability 0 come last, and the nucleus may be any size from 1 to the vocabulary.  The token is drawn among the kept
        words and `logp` is its log-probability under the kept, renormalised distribution.  top_p = 1 (the default) switches
        the filter off -- it is not a nucleus of mass 1 -- and is the call without the keyword, launch for launch; valid
        values are 0 < top_p <= 1 (st_rnn_sample_topp).

        Returns (ids (B, S, T) int64, 0 after <end>; logp (B, S, T) fp32, the log-probability of each token under the
        distribution it was drawn from, 0 after <end>; lengths (B, S) int64 counting <end>, T if <end> was never drawn)."""
        B, S, T = self._sample_shape(cnn_feature, num_samples, temperature, top_k, max_length, uniforms, top_p)
        with torch.no_grad():
            prm, keep = self._c_params()
            if not cnn_feature.is_cuda:
                raise _lib.ShowTellHipError("cnn_feature must be on the HIP device (no CPU fallback)")
            feat, n, u, ids, logp = self._sample_buffers(self._feature(cnn_feature), B, S, T, uniforms, generator)
            nbytes = lib().st_rnn_sample_workspace_bytes(C.byref(prm), n)
            ws = torch.empty(nbytes, device=feat.device, dtype=torch.uint8)
            if top_p == 1.0:
                check(lib().st_rnn_sample(C.byref(prm), _cp(feat), n, T, _cp(u), 1.0 / float(temperature), int(top_k), int(end_id), _cp(ws),
                                          nbytes, _cp(ids), _cp(logp), _stream()), "st_rnn_sample")
            else:
                check(lib().st_rnn_sample_topp(C.byref(prm), _cp(feat), n, T, _cp(u), 1.0 / float(temperature), int(top_k), float(top_p),
                                               int(end_id), _cp(ws), nbytes, _cp(ids), _cp(logp), _stream()), "st_rnn_sample_topp")
            return ids.view(B, S, T), logp.view(B, S, T), sample_lengths(ids, end_id).view(B, S)

    def sentence_index(self, cnn_feature, beam_size=0, return_logits=False):
        """rnn.py:37-108: 25-step greedy decode (beam_size=0) or the bs=1 ranking loop (beam_size>0)."""
        if beam_size and beam_size > 0:
            from .beam import quirky_beam
            return quirky_beam(self, cnn_feature, beam_size)
        with torch.no_grad():
            prm, keep = self._c_params()
            feat = self._feature(cnn_feature)
            B = feat.shape[0]
            nbytes = lib().st_rnn_greedy_workspace_bytes(C.byref(prm), B)
            ws = torch.empty(nbytes, device=feat.device, dtype=torch.uint8)
            ids = torch.empty(B, CAP_MAX, device=feat.device, dtype=torch.long)
            lg = torch.empty(CAP_MAX, B, up8(self.vocab_size), device=feat.device) if return_logits else None
            check(lib().st_rnn_greedy(C.byref(prm), _cp(feat), B, CAP_MAX, _cp(ws), nbytes, _cp(ids), _cp(lg), _stream()),
                  "st_rnn_greedy")
        out = ids.squeeze()                                               # rnn.py:56
        if return_logits:
            return out, lg[:, :, :self.vocab_size].permute(1, 0, 2)
        return out
