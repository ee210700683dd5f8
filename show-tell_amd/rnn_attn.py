"""Soft-attention decoder: drop-in for ``Attention/rnn_attn.py`` (``Attention_Net``, ``RNN_Attn``) and,
through the ``cell`` switch, ``Attention/rnn_attn_LSTM.py``.

    logits, alphas = rnn(cnn_feature, image_caption, caption_size)    # (N_tok, V) packed rows, (B, T, P) zero padded
    ids            = rnn.sentence_index(cnn_feature, vocab)           # Long(B, 25)
    ids, alphas    = rnn.sentence_index(cnn_feature, vocab, return_alphas=True)   # + (B, 25, P) attention maps
    hyps           = rnn.beam_search(cnn_feature, beam_width=5, return_alphas=True)   # per image [(tokens, cost, (len-1, P))]
    ids, logp, lengths, alphas = rnn.sample(cnn_feature, num_samples=5, return_alphas=True)   # (B, S, 25) draws + (B, S, 25, P) maps

Same constructor, attribute names (``embeddings, unit, linear, init_h, attn.{encoder_att, decoder_att,
full_att}, embed`` [+ ``init_c``]) and ``state_dict`` keys as the reference; the sub-modules are parameter
containers, the arithmetic runs in st_attn_forward / st_attn_backward / st_attn_greedy / st_attn_beam_search / st_attn_sample.

Reference quirks kept: the input token at step t is ``caption[:, t]`` (the same token
that is the target of that step), the initial hidden state is replicated over all layers, attention is keyed
on the last layer's state, ``alphas`` stay zero beyond each caption's length, unlike the reference the
module does not hard-code ``.cuda()`` but still requires a HIP device.
"""
import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._lib import AttnGrads, AttnParams, BeamOpts, check, dtype_code, lib, ref
from ._lib import ptr as _cp, stream as _stream
from .rnn import (CAP_MAX, Decoder, ce_loss, ce_loss_backward, check_caption_args, check_input_ids, check_label_smoothing,
                  check_weight_args, logits_grad, loss_terms, pack_row_weights, sample_lengths, scheduled_loss_inputs, unpack_rows, up8)
from .dropout import DropoutState
from .seq import plan_for


class Attention_Net(nn.Module):
    """Parameter container with the reference's attribute names (rnn_attn.py:13-19)."""

    def __init__(self, nos_filters, num_hidden_units, attention_dim=512):
        super(Attention_Net, self).__init__()
        self.encoder_att = nn.Linear(nos_filters, attention_dim)
        self.decoder_att = nn.Linear(num_hidden_units, attention_dim)
        self.full_att = nn.Linear(attention_dim, 1)
        self.relu = nn.LeakyReLU(negative_slope=0.2)
        self.softmax = nn.Softmax(dim=1)

    def forward(self, img_feat, hidden_state):  # pragma: no cover - container
        raise _lib.ShowTellHipError("Attention_Net is a parameter container; call RNN_Attn.forward")


class _AttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, _anchor, module, caption, lens, mode, alpha_c, need_grad, sequence_weight, token_weight, eps=0.0, input_ids=None):
        m = module
        dev = feat.device
        if not feat.is_cuda or not m.linear.weight.is_cuda:
            raise _lib.ShowTellHipError("the attention decoder and its inputs must live on a HIP device (no CPU fallback)")
        plan = plan_for(lens, dev)
        caption = caption.contiguous()
        seq = plan.c_struct(caption)
        # the kernels embed caption_T; with input_ids (scheduled sampling) that is the mixed ids, and the targets below stay the caption's
        cap_T = (caption if input_ids is None else input_ids.detach()).t().contiguous()
        prm, keep = m._c_params()
        dt = m.compute_dtype
        B, Fd, P = feat.shape
        if Fd != m.nos_filters or P != m.num_pixels_checked(P):
            raise _lib.ShowTellHipError(f"cnn_feature must be (B, {m.nos_filters}, P), got {tuple(feat.shape)}")
        prm.P = P
        featc = feat.detach().float().contiguous()
        nbytes = lib().st_attn_workspace_bytes(C.byref(prm), C.byref(seq))
        ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        V, Vp, n, T = m.vocab_size, up8(m.vocab_size), plan.ntok, caption.shape[1]
        alphas = torch.zeros(B, T, P, device=dev, dtype=torch.float32)        # rnn_attn.py:65
        roww = pack_row_weights(plan, sequence_weight, token_weight, dev)
        logits = torch.empty(n, Vp, device=dev, dtype=dt if mode == "loss" else torch.float32)
        # dropout in front of `linear`: forward() and loss() in train(); token_logp ('nll') scores the deterministic model
        took = None if mode == "nll" else m._dropout.take(m.training)
        drop = dbuf = None
        if took is not None:
            drop, dbuf = m._dropout.desc(took, lib().st_attn_dropout_bytes(C.byref(prm), C.byref(seq)), dev)
        check(lib().st_attn_forward(C.byref(prm), C.byref(seq), _cp(featc), _cp(cap_T), _cp(ws), nbytes, _cp(logits), dtype_code(logits.dtype),
                                    Vp, _cp(alphas), int(need_grad), ref(drop), _stream()), "st_attn_forward")
        ctx.drop, ctx.dbuf = drop, dbuf
        # st_attn_forward steps over plan.T columns; alphas has T (padded) columns: strides must agree
        ctx.m, ctx.plan, ctx.caption, ctx.cap_T, ctx.ws, ctx.mode, ctx.P = m, plan, caption, cap_T, ws, mode, P
        ctx.alphas, ctx.alpha_c, ctx.keep, ctx.roww = alphas, alpha_c, keep, roww
        if mode == "logits":
            return logits[:, :V], alphas
        targets = torch.nn.utils.rnn.pack_padded_sequence(caption, lens, batch_first=True)[0].contiguous()   # main_attn.py:126
        if mode == "nll":
            nll = torch.empty(n, device=dev, dtype=torch.float32)
            ce_loss(logits, logits.dtype, targets, n, V, Vp, None, loss_terms(nll=nll))
            ctx.mark_non_differentiable(nll, alphas)
            return nll, alphas
        loss = torch.zeros((), device=dev, dtype=torch.float32)
        ctx.terms = loss_terms(roww, None, eps)
        ce_loss(logits, dt, targets, n, V, Vp, loss, ctx.terms)           # the doubly-stochastic term below stays unweighted and unsmoothed
        check(lib().st_attn_reg_loss(_cp(alphas), B, T, P, float(alpha_c), _cp(loss), _stream()), "st_attn_reg_loss")
        ctx.logits, ctx.targets = logits, targets
        return loss, alphas

    @staticmethod
    def backward(ctx, g0, galphas):
        m, plan = ctx.m, ctx.plan
        dt = m.compute_dtype
        V, Vp, n = m.vocab_size, up8(m.vocab_size), plan.ntok
        gs = None
        dal = None
        if ctx.mode == "logits":
            dlog = logits_grad(g0, dt, n, V, Vp, torch.empty)
            dal = (galphas if galphas is not None else torch.zeros_like(ctx.alphas)).float().contiguous()
            alpha_c = 0.0
        elif ctx.mode != "loss":
            raise _lib.ShowTellHipError("token_logp has no gradient")
        else:
            dlog, gs = ce_loss_backward(ctx.logits, dt, ctx.targets, n, V, Vp, g0, ctx.terms)
            alpha_c = ctx.alpha_c
        prm, keep = m._c_params()
        prm.P = ctx.P
        grads, keep2 = m._c_grads()
        seq = plan.c_struct(ctx.caption)
        check(lib().st_attn_backward(C.byref(prm), C.byref(grads), C.byref(seq), _cp(ctx.cap_T), _cp(dlog), Vp, _cp(ctx.alphas), _cp(dal),
                                     float(alpha_c), _cp(gs), _cp(ctx.ws), ctx.ws.numel(), ref(ctx.drop), _stream()), "st_attn_backward")
        ctx.ws = ctx.dbuf = None
        return None, None, None, None, None, None, None, None, None, None, None, None


class RNN_Attn(Decoder):

    def __init__(self, embed_dim, nos_filters, attention_dim, num_hidden_units, vocab_size, num_layers, dtype=torch.float32,
                 dropout_out=0.0):
        '''
        Args (as the reference, rnn_attn.py:35-42) + dtype (kernel storage type) + dropout_out: nn.Dropout(p) in front of `linear`,
        the Show-Attend-Tell placement.  The recurrence and the next step's attention read the plain top state; only the vocabulary
        projection (and its weight gradient) sees the dropped copy.  Active only while ``self.training``, in ``forward()`` and
        ``loss()``; ``token_logp``, ``sentence_index``, ``beam_search`` and ``sample`` always run the deterministic model.  With
        p = 0, or in ``eval()``, each call is the launch sequence it was.  Seed and step counter: ``seed_dropout``.
        '''
        super(RNN_Attn, self).__init__()
        self._dropout = DropoutState(0.0, 0.0, dropout_out, num_layers)
        if num_layers > _lib.ST_MAX_LAYERS:
            raise ValueError(f"num_layers={num_layers} exceeds the kernel limit of {_lib.ST_MAX_LAYERS}")
        self.nos_filters = nos_filters
        self.num_layers = num_layers
        self.vocab_size = vocab_size
        self.embeddings = nn.Embedding(vocab_size, embed_dim)
        unit_cls = nn.GRU if self.cell == "gru" else nn.LSTM
        self.unit = unit_cls(2 * embed_dim, num_hidden_units, num_layers, batch_first=True)
        self.linear = nn.Linear(num_hidden_units, vocab_size)
        self.cap_max_size = CAP_MAX                                          # rnn_attn.py:53
        self.init_h = nn.Linear(nos_filters, num_hidden_units)
        if self.cell != "gru":
            self.init_c = nn.Linear(nos_filters, num_hidden_units)           # rnn_attn_LSTM.py:55
        self.attn = Attention_Net(nos_filters, num_hidden_units, attention_dim)
        self.embed = nn.Linear(nos_filters, embed_dim)
        self.embed_dim, self.hidden, self.attention_dim = embed_dim, num_hidden_units, attention_dim
        self.compute_dtype = dtype

    def num_pixels_checked(self, P):
        if P > 64:
            raise _lib.ShowTellHipError(f"at most 64 feature-map pixels are supported (got {P})")
        return P

    def _c_params(self):
        p, keep = AttnParams(), []
        wc = self._rnn_params(p.rnn, 2 * self.embed_dim, keep)
        p.F, p.A, p.P = self.nos_filters, self.attention_dim, 0      # every caller sets P from its feature map; 0 is rejected
        a = self.attn
        p.w_enc, p.b_enc = wc(a.encoder_att.weight), a.encoder_att.bias.data.data_ptr()
        p.w_dec, p.b_dec = wc(a.decoder_att.weight), a.decoder_att.bias.data.data_ptr()
        p.w_full, p.b_full = a.full_att.weight.data.data_ptr(), a.full_att.bias.data.data_ptr()
        p.w_init_h, p.b_init_h = wc(self.init_h.weight), self.init_h.bias.data.data_ptr()
        if self.cell != "gru":
            p.w_init_c, p.b_init_c = wc(self.init_c.weight), self.init_c.bias.data.data_ptr()
        p.w_embed, p.b_embed = wc(self.embed.weight), self.embed.bias.data.data_ptr()
        return p, keep

    def _c_grads(self):
        g, keep = AttnGrads(), []
        gb = self._rnn_grads(g.rnn, keep)
        a = self.attn
        g.w_enc, g.b_enc = gb(a.encoder_att.weight), gb(a.encoder_att.bias)
        g.w_dec, g.b_dec = gb(a.decoder_att.weight), gb(a.decoder_att.bias)
        g.w_full, g.b_full = gb(a.full_att.weight), gb(a.full_att.bias)
        g.w_init_h, g.b_init_h = gb(self.init_h.weight), gb(self.init_h.bias)
        if self.cell != "gru":
            g.w_init_c, g.b_init_c = gb(self.init_c.weight), gb(self.init_c.bias)
        g.w_embed, g.b_embed = gb(self.embed.weight), gb(self.embed.bias)
        return g, keep

    def _sched_inputs(self, cnn_feature, cap, lens, max_len, u, p, inv_t, top_k, ids, replaced):
        prm, keep, featc, B, P = self._decode_inputs(cnn_feature)
        T = cap.shape[1]
        cap_T = cap.t().contiguous()
        nbytes = lib().st_attn_sched_inputs_workspace_bytes(C.byref(prm), B)
        ws = torch.empty(nbytes, device=featc.device, dtype=torch.uint8)
        check(lib().st_attn_sched_inputs(C.byref(prm), _cp(featc), B, _cp(cap), _cp(cap_T), T, _cp(lens), max_len, _cp(u[0]), _cp(u[1]), p, inv_t,
                                         top_k, _cp(ws), nbytes, _cp(ids), _cp(replaced), None, None, _stream()), "st_attn_sched_inputs")

    def forward(self, cnn_feature, image_caption, caption_size, input_ids=None):
        """rnn_attn.py:98-118: (packed logits (N_tok,V) fp32, alphas (B,T,P)).  `input_ids` (B, T) int64 (``scheduled_inputs``):
        the token step t embeds, input_ids[b, t], in place of the caption's; None is the call it was."""
        if input_ids is None:
            return _AttnFn.apply(cnn_feature, self.linear.bias, self, image_caption, caption_size, "logits", 0.0, torch.is_grad_enabled(), None, None)
        check_input_ids(input_ids, image_caption, self.vocab_size)
        return _AttnFn.apply(cnn_feature, self.linear.bias, self, image_caption, caption_size, "logits", 0.0, torch.is_grad_enabled(), None, None,
                             0.0, input_ids)

    def loss(self, cnn_feature, image_caption, caption_size, alpha_c=1.0, sequence_weight=None, token_weight=None, label_smoothing=0.0,
             input_ids=None, scheduled_sampling=0.0, ss_temperature=1.0, ss_top_k=0, ss_generator=None, ss_uniforms=None):
        """main_attn.py:126-131 fused: CE(packed logits, packed caption) + alpha_c * mean((1 - sum_t alpha)^2).
        `sequence_weight` (B,) / `token_weight` (B, T) weight the cross-entropy terms as in RNN.loss (the divisor stays N_tok, no
        gradient into the weights); `label_smoothing` in [0, 1) smooths them as CrossEntropyLoss(label_smoothing=) does (0: the
        call it was); the doubly-stochastic term stays unweighted and unsmoothed.
        `input_ids` / `scheduled_sampling` (+ ss_*): as in RNN.loss -- the steps embed the mixed ids, the targets stay the caption,
        the embedding gradient goes to the tokens that were fed; the roll-in runs without dropout, this pass with it as usual."""
        eps = check_label_smoothing(label_smoothing)
        input_ids = scheduled_loss_inputs(self, cnn_feature, image_caption, caption_size, input_ids, scheduled_sampling, ss_temperature,
                                          ss_top_k, ss_generator, ss_uniforms)
        if sequence_weight is not None or token_weight is not None:
            check_caption_args(image_caption, caption_size)
            check_weight_args(image_caption.shape[0], image_caption.shape[1], sequence_weight, token_weight)
        if input_ids is None:
            out, _ = _AttnFn.apply(cnn_feature, self.linear.bias, self, image_caption, caption_size, "loss", float(alpha_c),
                                   torch.is_grad_enabled(), sequence_weight, token_weight, eps)
        else:
            out, _ = _AttnFn.apply(cnn_feature, self.linear.bias, self, image_caption, caption_size, "loss", float(alpha_c),
                                   torch.is_grad_enabled(), sequence_weight, token_weight, eps, input_ids)
        return out

    def token_logp(self, cnn_feature, image_caption, caption_size, input_ids=None):
        """log p(image_caption[b, t]) at every step of the teacher-forced pass (rnn_attn.py:98-118): (B, T) fp32, 0 past
        caption_size[b]; no gradient.  -token_logp.sum() / N_tok is the cross-entropy part of loss().  `input_ids`: as in ``forward``."""
        check_caption_args(image_caption, caption_size)
        if input_ids is not None:
            check_input_ids(input_ids, image_caption, self.vocab_size)
        with torch.no_grad():
            nll, _ = _AttnFn.apply(cnn_feature, self.linear.bias, self, image_caption, caption_size, "nll", 0.0, False, None, None, 0.0,
                                   input_ids)
            return unpack_rows(plan_for(caption_size, nll.device), -nll, image_caption.shape[1], nll.device)

    def _decode_inputs(self, cnn_feature):
        if not cnn_feature.is_cuda:
            raise _lib.ShowTellHipError("cnn_feature must be on the HIP device (no CPU fallback)")
        prm, keep = self._c_params()
        B, Fd, P = cnn_feature.shape
        prm.P = self.num_pixels_checked(P)
        return prm, keep, cnn_feature.detach().float().contiguous(), B, P

    def sentence_index(self, cnn_feature, vocab, return_alphas=False):
        """rnn_attn.py:120-145: greedy decode from vocab('<start>'), exactly cap_max_size steps.  With `return_alphas`,
        (ids, alphas): alphas (B, cap_max_size, P) fp32 on the device, the attention map of every step."""
        ind = vocab('<start>')                                               # rnn_attn.py:127
        with torch.no_grad():
            prm, keep, featc, B, P = self._decode_inputs(cnn_feature)
            nbytes = lib().st_attn_greedy_workspace_bytes(C.byref(prm), B)
            ws = torch.empty(nbytes, device=featc.device, dtype=torch.uint8)
            ids = torch.empty(B, self.cap_max_size, device=featc.device, dtype=torch.long)
            if return_alphas:
                alphas = torch.empty(B, self.cap_max_size, P, device=featc.device, dtype=torch.float32)
                check(lib().st_attn_greedy_alphas(C.byref(prm), _cp(featc), B, self.cap_max_size, int(ind), _cp(ws), nbytes, _cp(ids),
                                                  _cp(alphas), _stream()), "st_attn_greedy_alphas")
                return ids.squeeze(), alphas
            check(lib().st_attn_greedy(C.byref(prm), _cp(featc), B, self.cap_max_size, int(ind), _cp(ws), nbytes, _cp(ids), _stream()),
                  "st_attn_greedy")
        return ids.squeeze()                                                 # rnn_attn.py:143

    def sample(self, cnn_feature, num_samples=1, temperature=1.0, top_k=0, max_length=CAP_MAX, start_id=1, end_id=2,
               generator=None, uniforms=None, return_alphas=False, top_p=1.0):
        """The loop of rnn_attn.py:120-145 (test branch 77-94) from `start_id` with a draw in place of the arg-max of
        rnn_attn.py:141; arguments and results as RNN.sample (one st_attn_sample call for all B * num_samples rows).
        With `return_alphas` also alphas (B, S, T, P) fp32 on the device: the attention map of every step.
        `top_p` < 1 is the nucleus filter of RNN.sample, same rule and same order (temperature, top_k, top_p): a word is kept
        iff the mass strictly before it, value descending and the lowest index first among equals, is below top_p; `logp` is
        renormalised over the kept words; top_p = 1 is the filter off and the call without the keyword (st_attn_sample_topp)."""
        B, S, T = self._sample_shape(cnn_feature, num_samples, temperature, top_k, max_length, uniforms, top_p)
        with torch.no_grad():
            prm, keep, featc, B, P = self._decode_inputs(cnn_feature)
            featc, n, u, ids, logp = self._sample_buffers(featc, B, S, T, uniforms, generator)
            dev = featc.device
            nbytes = lib().st_attn_sample_workspace_bytes(C.byref(prm), n)
            ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
            alphas = torch.empty(n, T, P, device=dev, dtype=torch.float32) if return_alphas else None
            if top_p == 1.0:
                check(lib().st_attn_sample(C.byref(prm), _cp(featc), n, T, int(start_id), _cp(u), 1.0 / float(temperature), int(top_k),
                                           int(end_id), _cp(ws), nbytes, _cp(ids), _cp(logp), _cp(alphas), _stream()), "st_attn_sample")
            else:
                check(lib().st_attn_sample_topp(C.byref(prm), _cp(featc), n, T, int(start_id), _cp(u), 1.0 / float(temperature), int(top_k),
                                                float(top_p), int(end_id), _cp(ws), nbytes, _cp(ids), _cp(logp), _cp(alphas), _stream()),
                      "st_attn_sample_topp")
            out = (ids.view(B, S, T), logp.view(B, S, T), sample_lengths(ids, end_id).view(B, S))
            return out + (alphas.view(B, S, T, P),) if return_alphas else out

    def beam_search(self, cnn_feature, beam_width=4, num_hypotheses=1, max_length=50, start_id=1, end_id=2, return_alphas=False,
                    return_records=False, min_length=0, no_repeat_ngram_size=0, suppress_tokens=None, length_penalty=0.0,
                    num_beam_groups=1, diversity_penalty=0.0):
        """beam_search.py:45-97 for every image of the batch, driven by the test branch of rnn_attn.py:77-94: the root holds
        start_id with h0 = init_h(mean feature) over all layers (and c0 for the LSTM); a node's successors come from one step
        fed with the node's token, attention keyed on its top-layer state.  The whole search is one st_attn_beam_search call
        and one device-to-host copy of its records; the Node bookkeeping is replayed on the host (beam.replay_hypotheses).

        Returns, per image, at most `num_hypotheses` (tokens, cost) pairs, as RNN.beam_search ([] when nothing ended in time).
        With `return_alphas`: (tokens, cost, alphas), alphas a CPU float32 tensor (len(tokens) - 1, P) holding the extras of
        the nodes after the root: the attention map computed while producing each token.
        With `return_records`: (hypotheses, records), records the search's own numpy arrays dict(tok, cost, par
        [max_length+1][B][W], end [max_length][B][W]) and, with `return_alphas`, alpha [max_length][B*W][P]; a constrained
        search that keeps paths (max_length + 1 <= 64) adds hist [B][W][max_length+1] int32, the path of every slot of the last
        fringe as the search itself kept it.
        `min_length`, `no_repeat_ngram_size`, `suppress_tokens` and `length_penalty` constrain the search as in
        RNN.beam_search (beam.py); they travel in the call's st_beam_opts.
        `num_beam_groups` = G > 1 is diverse beam search as in RNN.beam_search (beam.py's docstring has the rule), the same
        st_attn_beam_search call; the hypotheses are then, per image, a list of G lists (each entry with its alphas under
        `return_alphas`), the records keep their layout (beam.group_records cuts a group out) and hist is handed out whenever
        the paths fit (max_length + 1 <= 64).  With G = 1 the result is that of the single beam."""
        from .beam import ST_BEAM_MAX_HIST, BeamConstraints, check_groups, replay_groups, replay_hypotheses
        if not 1 <= beam_width <= 8:
            raise ValueError(f"beam_width must be 1..8 (got {beam_width})")
        if max_length < 1:
            raise ValueError(f"max_length must be >= 1 (got {max_length})")
        G, lam = check_groups(beam_width, self.vocab_size, num_beam_groups, diversity_penalty)
        bc = BeamConstraints(self.vocab_size, max_length, min_length, no_repeat_ngram_size, suppress_tokens, length_penalty)
        with torch.no_grad():
            prm, keep, featc, B, P = self._decode_inputs(cnn_feature)
            W, T = beam_width, max_length
            n = B * W
            keep_paths = bc.keep_paths or (G > 1 and T + 1 <= ST_BEAM_MAX_HIST)
            opts = None                                                                # the plain search
            if G > 1 or bc.active:
                sup, n_sup = bc.suppress_on(featc.device)
                bo = BeamOpts(bc.min_length, bc.ngram, _cp(sup), n_sup, int(keep_paths), G, lam)
                opts = C.byref(bo)
            paths_at = C.c_size_t(0)
            nbytes = lib().st_attn_beam_workspace_bytes(C.byref(prm), B, W, T, opts, C.byref(paths_at))
            ws = torch.empty(nbytes, device=featc.device, dtype=torch.uint8)
            # the records share one buffer, so that the search ends in ONE device-to-host copy
            layout = [("tok", torch.long, (T + 1, B, W)), ("cost", torch.float32, (T + 1, B, W)), ("par", torch.int32, (T + 1, B, W)),
                      ("end", torch.uint8, (T, B, W))]
            if return_alphas:
                layout.append(("alpha", torch.float32, (T, n, P)))
            offs, o = {}, 0
            for name, dt, shape in layout:
                nb = int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
                offs[name] = (o, nb)
                o += (nb + 255) // 256 * 256
            rec = torch.empty(o, device=featc.device, dtype=torch.uint8)
            view = {name: rec[offs[name][0]:offs[name][0] + offs[name][1]].view(dt).view(shape) for name, dt, shape in layout}
            check(lib().st_attn_beam_search(C.byref(prm), _cp(featc), B, W, T, int(start_id), int(end_id), _cp(ws), nbytes,
                                            _cp(view["tok"]), _cp(view["cost"]), _cp(view["par"]), _cp(view["end"]),
                                            _cp(view.get("alpha")), opts, _stream()), "st_attn_beam_search")
            host = rec.cpu().numpy()
            hist = None
            if return_records and keep_paths:                                      # the last fringe's path buffer, where the planner put it
                off, nb = paths_at.value, n * (T + 1) * 4
                hist = ws[off:off + nb].view(torch.int32).view(B, W, T + 1).cpu().numpy()
        npdt = {torch.long: np.int64, torch.float32: np.float32, torch.int32: np.int32, torch.uint8: np.uint8}
        h = {name: host[offs[name][0]:offs[name][0] + offs[name][1]].view(npdt[dt]).reshape(shape) for name, dt, shape in layout}
        if G > 1:
            hyps = replay_groups(h, G, num_hypotheses, bc.length_penalty)
        else:
            hyps = replay_hypotheses(h["tok"], h["cost"], h["par"], h["end"], num_hypotheses, h.get("alpha"), bc.length_penalty)
        if hist is not None:
            h["hist"] = hist
        return (hyps, h) if return_records else hyps
