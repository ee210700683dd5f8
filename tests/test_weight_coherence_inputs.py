"""Inputs of the weight-coherence tests (tests/test_gpu_weight_coherence.py imports the builders, the weight changes and
the oracle from here), and the proof, from the float64 oracle alone, that these inputs can catch a stale weight copy.
Nothing here needs a GPU.

The GPU tests build a model on weights W0, run it (so that every derived copy of the weights is cached), change the
weights to W1 by some path and compare the next run with the float64 oracle on W1.  A kernel that still read a copy of W0
would produce the oracle's value on W0 -- so the test has power only if the oracle on W0 and the oracle on W1 differ by
much more than the bound the kernels are held to.  The condition asserted here for every case of the GPU file:

    each checked output differs between the oracle on W0 and the oracle on W1 by at least POWER = 20 x its bound,
    measured with the same error function the GPU test applies.

Decoder outputs and bounds (tests/test_gpu_decoder_bench_shape.py): loss (LOSS_REL), logits (GRAD_L2, GRAD_MAX), d loss /
d feat per row (ROW_L2; the attention decoders return no feature gradient: loss and logits only).  Encoder outputs
(tests/test_gpu_encoder.py, TOL[bfloat16] in the max norm): pooled features and head output of cnn.ResNet, the feature map
of cnn_attn.ResNet.

How W1 is chosen.  Whole-model cases: another seed, with the vocabulary projection (decoders) / the last stage's BatchNorm
gains and biases (encoder) at another scale, so that loss and output scale differ, not only the direction.  Single-tensor
cases: the tensor re-drawn from another seed at SCALE[op] x its scale ("load", "copy"), negated ("neg": p.mul_(-1)) or
drawn in place by nn.init.normal_ at its own scale ("normal"; the GPU test draws on the device, here the same distribution
is drawn on the host).  Where a change cannot be relied on to move an output by 20 x its bound, the case claims power on the
outputs it does move (POWERED_EXTRA and decoder_powered, the ENC_* comment): the GPU test still holds every output to its bound.

`python -m tests.test_weight_coherence_inputs` prints the gap of every case and output as a multiple of its bound."""
import functools

import pytest
import torch

from oracle import restatement as R
from tests._util import _bf16
from tests.test_gpu_decoder_bench_shape import GRAD_L2, GRAD_MAX, LOSS_REL, ROW_L2, _captions, _rel_l2, _rel_max, _row_l2

POWER = 20.0
ENC_TOL = 6e-2                 # tests/test_gpu_encoder.py: TOL[torch.bfloat16], max |got - ref| / max |ref|
BOUNDS = {"loss": LOSS_REL, "logits_l2": GRAD_L2, "logits_max": GRAD_MAX, "dfeat_rows": ROW_L2,
          "pooled": ENC_TOL, "head": ENC_TOL, "map": ENC_TOL}

FAMILIES = ("gru", "lstm", "attn_gru", "attn_lstm")
PLAIN = dict(E=64, H=64, L=2, V=300, lens=[6, 5, 5, 3, 2])
ATTN = dict(E=32, F=48, A=40, H=64, V=50, L=3, P=49, lens=[9, 6, 6, 4])      # tests/golden/attn_*_small.npz
# scale of linear.weight / of the cells' matrices: a default-initialised decoder is nearly uniform over the vocabulary and
# its loss ~ log V whatever the weights are (tests/test_gpu_decoder_bench_shape.py, case A)
SHARP = {("gru", 0): dict(lin=6.0, rec=2.0), ("gru", 1): dict(lin=16.0, rec=2.0),
         ("lstm", 0): dict(lin=30.0, rec=3.0), ("lstm", 1): dict(lin=10.0, rec=3.0)}
# attention decoders, W0 and W1 alike: peaked attention (attn.full_att.weight, tests/test_gpu_attention_bench_shape.py), scores
# in which the hidden state's term (decoder_att) is comparable to the features' (encoder_att), and an input in which the
# attended feature (embed) weighs as much as the token -- else no change of the attention's own matrices moves the logits
ATTN_SCALE = {"attn.full_att.weight": 8.0, "attn.decoder_att.weight": 16.0, "attn.encoder_att.weight": 4.0, "embed.weight": 4.0}
SEEDS = {0: 11, 1: 12}
OPS = ("load", "copy", "neg", "normal")
DEC_REDRAW = 2.0               # single decoder tensors are re-drawn at twice their scale ("load", "copy")
NORMAL_SCALE = 1.0             # nn.init.normal_ draws at the tensor's own scale


def cell_of(family):
    return "lstm" if family.endswith("lstm") else "gru"


def is_attn(family):
    return family.startswith("attn")


def geometry(family):
    return ATTN if is_attn(family) else PLAIN


@functools.lru_cache(maxsize=None)
def _decoder_params(family, which):
    g, s = geometry(family), SHARP[(cell_of(family), which)]
    attn = dict(F=g["F"], A=g["A"]) if is_attn(family) else None
    p = R.init_decoder_params(g["E"], g["H"], g["V"], g["L"], cell_of(family), seed=SEEDS[which], attn=attn)
    p = {k: v.clone() for k, v in p.items()}
    p["linear.weight"] *= s["lin"]
    for k in p:
        if k.startswith("unit.weight"):
            p[k] *= s["rec"]
    if attn:
        for k, scale in ATTN_SCALE.items():
            p[k] *= scale
    return {k: _bf16(v) for k, v in p.items()}


def decoder_params(family, which):
    """bf16-representable parameters W0 (which = 0) or W1 (1) of the family's decoder; a fresh dict of clones"""
    return {k: v.clone() for k, v in _decoder_params(family, which).items()}


@functools.lru_cache(maxsize=None)
def _decoder_batch(family, batch):
    g = geometry(family)
    gen = torch.Generator().manual_seed(100 + batch)
    if is_attn(family):
        gain = 0.75 + 0.5 * torch.rand(len(g["lens"]), 1, g["P"], generator=gen)
        feat = torch.randn(len(g["lens"]), g["F"], g["P"], generator=gen).abs() * gain
    else:
        feat = torch.randn(len(g["lens"]), g["E"], generator=gen)
    cap, lens = _captions(g["lens"], g["V"], seed=100 + batch)
    return _bf16(feat), cap, lens


def decoder_batch(family, batch=0):
    """(feat, caption, lengths) of the family's geometry; `batch` numbers independent minibatches"""
    return _decoder_batch(family, batch)


def single_tensors(family):
    """the tensors a decoder's kernels read through a cached bf16 working copy"""
    g = geometry(family)
    names = ["embeddings.weight"] + [f"unit.weight_{w}_l{l}" for l in range(g["L"]) for w in ("ih", "hh")] + ["linear.weight"]
    if is_attn(family):
        names += ["attn.encoder_att.weight", "attn.decoder_att.weight", "init_h.weight", "embed.weight"]
        if cell_of(family) == "lstm":
            names.append("init_c.weight")
    return names


def redraw_std(v, scale=DEC_REDRAW):
    """standard deviation at which a tensor is re-drawn: `scale` x its own"""
    return float(v.float().std() if v.numel() > 1 else v.float().abs().max()) * scale


def changed(params, names, op, seed=7, scale=DEC_REDRAW, normal_scale=NORMAL_SCALE):
    """W1 of a case: `params` with the tensors `names` changed as the operation `op` changes them.  bf16-representable for
    the deterministic operations (so that the fp32 masters on the GPU can be compared bit for bit).  "normal" is
    nn.init.normal_(p, 0, NORMAL_SCALE x std(p)): at N(0, 1) a 64-wide cell matrix is 8 x its initialisation scale, the gates
    saturate and the stack amplifies bf16 storage rounding beyond every bound (measured: logits up to 5.9e-2 in relative L2
    on correct, freshly cast weights; at twice the tensor's own scale the attention decoders still reached 1.3e-2, and the
    float64 oracle itself then moves its logits by 1.2e-2 under a 2^-9 relative perturbation of the weights) -- a property
    of those weights, as the x5 case of tests/test_gpu_decoder_bench_shape.py."""
    out = {k: v.clone() for k, v in params.items()}
    g = torch.Generator().manual_seed(seed)
    for k in names:
        v = params[k]
        if op == "neg":
            out[k] = -v
        elif op == "normal":
            out[k] = torch.randn(v.shape, generator=g) * redraw_std(v, normal_scale)
        else:
            out[k] = _bf16(torch.randn(v.shape, generator=g) * redraw_std(v, scale))
    return out


def kernel_view(params):
    """What the bf16 kernels read of fp32 masters `params`: the round-to-nearest bf16 of every matrix that has a working copy
    or a packed copy (dim >= 2), the fp32 values of everything read live (biases, BatchNorm, attn.full_att.weight)."""
    return {k: (_bf16(v) if v.is_floating_point() and v.dim() >= 2 and k != "attn.full_att.weight" else v.clone())
            for k, v in params.items()}


def decoder_oracle(family, params, batch=0):
    """float64 oracle of the decoder on the kernels' view of `params`: {loss, logits, dfeat}; dfeat is None for attention"""
    feat, cap, lens = decoder_batch(family, batch)
    po = {k: v.double() for k, v in kernel_view(params).items()}
    if is_attn(family):
        with torch.no_grad():
            lo, logits, _ = R.attn_train_loss(po, feat.double(), cap, lens, 1.0, cell_of(family))
        return dict(loss=lo.item(), logits=logits, dfeat=None)
    fo = feat.double().requires_grad_(True)
    lo, logits, _ = R.gru_train_loss(po, fo, cap, lens, cell_of(family))
    lo.backward()
    return dict(loss=lo.item(), logits=logits.detach(), dfeat=fo.grad)


def decoder_errors(got, ref):
    """{output: error} of `got` against `ref` (both as decoder_oracle returns them), by the functions the bounds belong to"""
    e = {"loss": abs(got["loss"] - ref["loss"]) / abs(ref["loss"]),
         "logits_l2": _rel_l2(got["logits"], ref["logits"]), "logits_max": _rel_max(got["logits"], ref["logits"])}
    if ref["dfeat"] is not None:
        e["dfeat_rows"] = _row_l2(got["dfeat"], ref["dfeat"])
    return e


# ---- encoder -----------------------------------------------------------------------------------------------------------

ENC_VERSION, ENC_EMBED, ENC_SHAPE = 18, 64, (2, 3, 64, 64)
# one convolution of each packing (st_resnet_conv_info of ResNet-18): the 7 x 7 stem; a 3 x 3 with a fragment-major second
# copy (ntw > 0), one in layer1 and one in layer3 (another tile count); a stride-2 3 x 3 without one; a downsample 1 x 1
# (ResNet-18's basic blocks have no other 1 x 1 convolution).  conv index in network order -> state_dict key
ENC_CONVS = {"stem7x7": (0, "model.0.weight"), "c3x3_frag": (1, "model.4.0.conv1.weight"),
             "c3x3_frag_l3": (13, "model.6.1.conv1.weight"), "c3x3_s2": (5, "model.5.0.conv1.weight"),
             "down1x1": (12, "model.6.0.downsample.0.weight")}
ENC_HEAD = "linear_secondlast_layer.weight"
ENC_LAST_STAGE_SCALE = {0: 1.0, 1: 1.0 / 3.0}
# The pooled features are >= 0 and the bound is a max norm relative to the oracle on W1: a change that only enlarges or
# re-directs them gives a gap of at most ~1 = 16.7 x the bound, whatever it does (measured: negating a convolution 3..14 x,
# N(0, 1) in its place 10..16 x).  A gap of 20 x needs features that SHRINK.  So W0 and W1 hold the case convolutions and the
# head's Linear at ENC_BIG x their initialisation scale, the single-tensor cases re-draw one of them at ENC_SHRINK x that
# (back to its initialisation scale), and in the two blocks whose case convolution has a parallel path (layer2.0: conv1
# beside the downsample; layer3.0: the downsample beside the branch) the other path's BatchNorm gain is ENC_OTHER_PATH x.
ENC_BIG, ENC_SHRINK, ENC_OTHER_PATH = 4.0, 0.25, 0.2
ENC_QUIET = ("model.5.0.downsample.1.weight", "model.6.0.bn2.weight")


@functools.lru_cache(maxsize=None)
def _encoder_params(which, damp):
    seed = 21 + which
    p = R.init_encoder_params(ENC_VERSION, ENC_EMBED, seed=seed)
    g = torch.Generator().manual_seed(seed + 100)
    for k in p:                          # non-trivial BN affine / running stats (tests/test_gpu_encoder.py); the residual branches
        bn = ".bn" in k or k.startswith(("model.1.", "last_layer.")) or "downsample.1" in k     # at full scale: 8 blocks only
        if k.endswith("running_mean"):
            p[k] = torch.randn(p[k].shape, generator=g) * 0.1
        elif k.endswith("running_var"):
            p[k] = torch.rand(p[k].shape, generator=g) + 0.5
        elif k.endswith(".weight") and bn:
            p[k] = torch.rand(p[k].shape, generator=g) * 0.5 + 0.75
            if damp and ".bn2." in k:
                p[k] = torch.rand(p[k].shape, generator=g) * 0.2 + 0.1
        elif k.endswith(".bias") and bn:
            p[k] = torch.randn(p[k].shape, generator=g) * 0.1
    s = ENC_LAST_STAGE_SCALE[which]
    for k in p:                          # the output scale of the backbone: gains and biases that feed the last residual sums
        if k.startswith(("model.7.0.bn2.", "model.7.0.downsample.1.", "model.7.1.bn2.")) and k.endswith((".weight", ".bias")):
            p[k] = p[k] * s
    for k in ENC_QUIET:
        p[k] = p[k] * ENC_OTHER_PATH
    for k in [v[1] for v in ENC_CONVS.values()] + [ENC_HEAD]:
        p[k] = p[k] * ENC_BIG
    for k in p:
        if p[k].dim() >= 2:
            p[k] = _bf16(p[k])
    return p


def encoder_params(which, damp=False):
    """W0 / W1 of the encoder.  damp: the residual branches' last BatchNorm gains in [0.1, 0.3] as tests/test_gpu_encoder.py
    sets them for bf16 -- the train-mode cases take these: batch statistics over the 8 samples per channel that two 64 x 64
    images leave in the last stage amplify storage rounding, and full-scale branches multiply that block after block"""
    return {k: v.clone() for k, v in _encoder_params(which, damp).items()}


@functools.lru_cache(maxsize=None)
def encoder_images(batch=0):
    return torch.randn(*ENC_SHAPE, generator=torch.Generator().manual_seed(200 + batch))


def encoder_oracle(params, train, attn=False, batch=0):
    """float64 oracle on the kernels' view of `params`: {pooled, head} of cnn.ResNet, {map} of cnn_attn.ResNet.  The running
    buffers of a train-mode forward are updated in a copy."""
    po = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in kernel_view(params).items()}
    x = encoder_images(batch).double()
    with torch.no_grad():
        if attn:
            return {"map": R.encoder_attn_forward(po, x, ENC_VERSION, train=train)}
        pooled = R.backbone_forward({k: v.clone() for k, v in po.items()}, x, ENC_VERSION, train=train, avgpool=True).flatten(1)
        return {"pooled": pooled, "head": R.encoder_forward(po, x, ENC_VERSION, train=train)}


def enc_rel(got, ref):
    """tests/test_gpu_encoder.py:_rel in float64"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-6)).item()


def encoder_errors(got, ref):
    return {k: enc_rel(got[k], ref[k]) for k in ref}


# ---- optimizer trajectories (P3) -----------------------------------------------------------------------------------------

P3_STEPS = 3
P3_HYPER = {"sgd": dict(lr=0.5, momentum=0.9), "adam": dict(lr=0.05)}


class Follower:
    """The fp32 masters of an optimizer run, followed in float64 (R.sgd_momentum_step / R.adam_step)."""

    def __init__(self, kind, params):
        self.kind, self.hyper = kind, P3_HYPER[kind]
        self.p = {k: v.double().clone() for k, v in params.items()}
        self.state, self.steps = {}, 0

    def step(self, grads):
        self.steps += 1
        for k, g in grads.items():
            g = g.double()
            if self.kind == "sgd":
                self.state[k] = R.sgd_momentum_step(self.p[k], g, self.state.get(k), self.hyper["lr"], self.hyper["momentum"])
            else:
                if k not in self.state:
                    self.state[k] = (torch.zeros_like(g), torch.zeros_like(g))
                R.adam_step(self.p[k], g, *self.state[k], self.steps, self.hyper["lr"])

    def masters(self):
        return {k: v.float() for k, v in self.p.items()}


def oracle_gradients(family, params, batch=0):
    """float64 parameter gradients of the training loss on the kernels' view of `params` (host-only stand-in for backward())"""
    feat, cap, lens = decoder_batch(family, batch)
    po = {k: v.double().requires_grad_(True) for k, v in kernel_view(params).items()}
    if is_attn(family):
        lo = R.attn_train_loss(po, feat.double(), cap, lens, 1.0, cell_of(family))[0]
    else:
        lo = R.gru_train_loss(po, feat.double(), cap, lens, cell_of(family))[0]
    lo.backward()
    return {k: v.grad for k, v in po.items()}


# ---- the cases and their power --------------------------------------------------------------------------------------------

def decoder_cases():
    """(family, op, name-or-None): every deterministic W0 -> W1 change the GPU file makes to a decoder.  None: all tensors."""
    out = []
    for f in FAMILIES:
        out.append((f, "seed", None))                     # whole model: W1 = decoder_params(f, 1)
        out += [(f, op, None) for op in ("neg", "normal")]          # P5 whole model (copy_ takes the "seed" W1)
        out += [(f, op, k) for k in single_tensors(f) for op in OPS]
    return out


def decoder_w1(family, op, name):
    w0 = decoder_params(family, 0)
    if op == "seed":
        return decoder_params(family, 1)
    names = [name] if name is not None else [k for k, v in w0.items() if v.is_floating_point()]
    return changed(w0, names, op)


# Outputs besides the logits' relative L2 on which a case reaches POWER with the host's draw, per family and tensor (None: every
# tensor at once), as "<op>:<letters>" with L = loss, M = logits in the max norm, D = d loss / d feat rows.  What is missing is
# what that change cannot be relied on to move: the loss is one scalar, which two decoders that differ in one matrix (or in
# sign, or in a draw at the same scale) may share to a few per cent, and the max norm gap saturates near 1 = 25 x GRAD_MAX.
# Every output is still held to its bound on the GPU.  (python -m tests.test_weight_coherence_inputs prints the figures.)
POWERED_EXTRA = {
    "gru": {
        None: "neg:MD normal:MD",
        'embeddings.weight': "load:MD copy:MD neg:MD normal:MD",
        'unit.weight_ih_l0': "load:MD copy:MD neg:MD normal:MD",
        'unit.weight_hh_l0': "load:D copy:D neg:D normal:",
        'unit.weight_ih_l1': "load:LMD copy:LMD neg:MD normal:MD",
        'unit.weight_hh_l1': "load:D copy:D neg:D normal:",
        'linear.weight': "load:LMD copy:LMD neg:MD normal:MD",
    },
    "lstm": {
        None: "neg:MD normal:MD",
        'embeddings.weight': "load:MD copy:MD neg:MD normal:LMD",
        'unit.weight_ih_l0': "load:LMD copy:LMD neg:MD normal:LMD",
        'unit.weight_hh_l0': "load:D copy:D neg:D normal:D",
        'unit.weight_ih_l1': "load:LMD copy:LMD neg:MD normal:MD",
        'unit.weight_hh_l1': "load:MD copy:MD neg:MD normal:MD",
        'linear.weight': "load:LMD copy:LMD neg:MD normal:MD",
    },
    "attn_gru": {
        None: "neg:LM normal:LM",
        'embeddings.weight': "load: copy: neg: normal:",
        'unit.weight_ih_l0': "load:LM copy:LM neg:M normal:LM",
        'unit.weight_hh_l0': "load: copy: neg: normal:",
        'unit.weight_ih_l1': "load:M copy:M neg:LM normal:M",
        'unit.weight_hh_l1': "load: copy: neg:M normal:",
        'unit.weight_ih_l2': "load:L copy:L neg:LM normal:M",
        'unit.weight_hh_l2': "load:M copy:M neg: normal:",
        'linear.weight': "load:LM copy:LM neg:LM normal:LM",
        'attn.encoder_att.weight': "load:M copy:M neg:M normal:M",
        'attn.decoder_att.weight': "load: copy: neg: normal:",
        'init_h.weight': "load:M copy:M neg:M normal:M",
        'embed.weight': "load:M copy:M neg:M normal:M",
    },
    "attn_lstm": {
        None: "neg:M normal:LM",
        'embeddings.weight': "load:M copy:M neg:M normal:M",
        'unit.weight_ih_l0': "load:M copy:M neg:LM normal:M",
        'unit.weight_hh_l0': "load: copy: neg: normal:",
        'unit.weight_ih_l1': "load:LM copy:LM neg:LM normal:LM",
        'unit.weight_hh_l1': "load:LM copy:LM neg:M normal:",
        'unit.weight_ih_l2': "load:LM copy:LM neg:M normal:M",
        'unit.weight_hh_l2': "load:LM copy:LM neg:M normal:M",
        'linear.weight': "load:LM copy:LM neg:M normal:M",
        'attn.encoder_att.weight': "load:M copy:M neg:M normal:M",
        'attn.decoder_att.weight': "load: copy: neg: normal:",
        'init_h.weight': "load:LM copy:LM neg:M normal:LM",
        'embed.weight': "load:LM copy:LM neg:LM normal:LM",
        'init_c.weight': "load:LM copy:LM neg:LM normal:M",
    },
}
_LETTERS = {"L": "loss", "M": "logits_max", "D": "dfeat_rows"}


def decoder_powered(family, op, name, device_draw=False):
    """The outputs on which a decoder case must have POWER: all of them for a whole model from another seed (None), else the
    logits in relative L2, which every tensor moves, and what POWERED_EXTRA lists.  device_draw: the case's values were
    drawn on the GPU by nn.init.normal_, not the host's stand-in draw the table was made with: the logits' L2 only."""
    if name is None and op == "seed":
        return None
    if op == "normal" and device_draw:
        return ("logits_l2",)
    extra = dict(part.split(":") for part in POWERED_EXTRA[family][name].split())[op]
    return ("logits_l2",) + tuple(_LETTERS[c] for c in extra)


ENC_BN = "bn"            # every BatchNorm2d gain and running variance at once (they are read live from the flat arrays)


ENC_MATRICES = "matrices"      # every convolution and the head's Linear at once: the tensors that have a derived copy


def encoder_names(key):
    """the state_dict keys a single-tensor encoder case changes"""
    if key == "head":
        return [ENC_HEAD]
    if key == ENC_MATRICES:
        return [k for k, v in _encoder_params(0, False).items() if v.dim() == 4] + [ENC_HEAD]
    return [ENC_CONVS[key][1]]


def encoder_cases():
    """(op, key): "seed": the whole encoder; one case convolution or the head's Linear re-drawn at ENC_SHRINK x its scale by
    load_state_dict ("load"), copy_ ("copy") or nn.init.normal_(w, 0, ENC_SHRINK x std(w)) ("normal"); the head also negated;
    ENC_MATRICES: nn.init.normal_ like that on every convolution and the head's Linear; ENC_BN: the BatchNorm gains and running
    variances of W1 in W0.  mul_(-1) on a convolution is left out: it cannot shrink the features (see ENC_BIG above;
    the oracle gap measured 3 .. 14 x the bound)."""
    out = [("seed", None), ("load", ENC_BN), ("normal", ENC_MATRICES)]
    out += [(op, key) for key in ENC_CONVS for op in ("load", "copy", "normal")]
    out += [(op, "head") for op in ("load", "copy", "neg", "normal")]
    return out


def encoder_w1(op, key):
    w0 = encoder_params(0)
    if op == "seed":
        return encoder_params(1)
    if key == ENC_BN:
        w1 = encoder_params(1)
        for k in w0:
            if k.startswith("model.") and (k.endswith("running_var") or (w0[k].dim() == 1 and k.endswith(".weight"))):
                w0[k] = w1[k]
        return w0
    return changed(w0, encoder_names(key), op, scale=ENC_SHRINK, normal_scale=ENC_SHRINK)


@functools.lru_cache(maxsize=None)
def decoder_w0_oracle(family):
    return decoder_oracle(family, decoder_params(family, 0))


@functools.lru_cache(maxsize=None)
def encoder_w0_oracle(train, attn):
    return encoder_oracle(encoder_params(0, damp=train), train, attn)


def decoder_power(family, op, name):
    """{output: gap / bound} between the oracle on W0 and on W1"""
    e = decoder_errors(decoder_w0_oracle(family), decoder_oracle(family, decoder_w1(family, op, name)))
    return {k: v / BOUNDS[k] for k, v in e.items()}


def encoder_power(op, key, train=False, attn=False):
    w1 = encoder_params(1, damp=True) if train else encoder_w1(op, key)
    e = encoder_errors(encoder_w0_oracle(train, attn), encoder_oracle(w1, train, attn))
    if key == "head":
        e.pop("pooled", None)            # the head's Linear does not feed the pooled features
    return {k: v / BOUNDS[k] for k, v in e.items()}


def _assert_power(case, mult, outputs=None):
    checked = 0
    for out, m in mult.items():
        if outputs is not None and out not in outputs:
            continue
        assert m >= POWER, (case, out, f"oracle gap W0 / W1 is {m:.1f} x the bound, below {POWER:.0f} x")
        checked += 1
    assert checked >= 1, (case, "no output with power")


@pytest.mark.parametrize("family,op,name", decoder_cases())
def test_decoder_cases_have_power(family, op, name):
    _assert_power((family, op, name), decoder_power(family, op, name), decoder_powered(family, op, name))


@pytest.mark.parametrize("op,key", encoder_cases())
def test_encoder_eval_cases_have_power(op, key):
    _assert_power(("cnn", op, key), encoder_power(op, key))


def test_encoder_train_and_attention_cases_have_power():
    _assert_power(("cnn", "seed", "train"), {k: v for k, v in encoder_power("seed", None, train=True).items() if k == "pooled"})
    _assert_power(("cnn_attn", "seed", None), encoder_power("seed", None, attn=True))


def trajectory_power(family, kind, start=0, steps=P3_STEPS):
    """([per step {output: gap / bound}], {output: gap / bound} over all steps, [oracle loss before each step and after the
    last]) of an oracle-only optimizer run from W<start> (its own float64 gradients in place of backward()'s).  As in the GPU
    test, step s trains on minibatch s and the weights it produces are checked on minibatch s + 1: the gap of step s is that
    between the weights before and after it, on minibatch s + 1; the overall gap is on the last minibatch."""
    fol = Follower(kind, decoder_params(family, start))
    first = fol.masters()
    per_step, losses = [], []
    for s in range(steps):
        before = fol.masters()
        losses.append(decoder_oracle(family, before, s)["loss"])
        fol.step(oracle_gradients(family, before, s))
        e = decoder_errors(decoder_oracle(family, before, s + 1), decoder_oracle(family, fol.masters(), s + 1))
        per_step.append({k: v / BOUNDS[k] for k, v in e.items()})
    last = decoder_oracle(family, fol.masters(), steps)
    losses.append(last["loss"])
    total = decoder_errors(decoder_oracle(family, first, steps), last)
    return per_step, {k: v / BOUNDS[k] for k, v in total.items()}, losses


@pytest.mark.parametrize("kind", sorted(P3_HYPER))
@pytest.mark.parametrize("family", FAMILIES)
def test_optimizer_trajectories_have_power(family, kind):
    """P3 / P4: every single optimizer step moves the logits of the next minibatch by 20 x GRAD_L2 (a working copy that lags one
    step behind is caught at the next forward; the scalar loss goes up and down along these large steps and may pass its
    earlier value), and the three steps together move every output, the loss included, by 20 x its bound (a copy that never
    follows, which is what shadow_dtype=None gave, is caught on each of them).  A fresh minibatch per step, as in training:
    three steps on ONE minibatch of random captions drive its loss towards zero, where a relative bound on it means nothing."""
    steps, total, _ = trajectory_power(family, kind)
    for s, m in enumerate(steps):
        _assert_power((family, kind, f"step {s}"), m, ("logits_l2",))
    _assert_power((family, kind, "all steps"), total)


@pytest.mark.parametrize("family", FAMILIES)
def test_one_step_from_w1_has_power(family):
    """P6 under a flat optimizer: the SGD step taken after the round trip moves the logits by 20 x GRAD_L2"""
    steps, _, _ = trajectory_power(family, "sgd", start=1, steps=1)
    _assert_power((family, "sgd", "one step from W1"), steps[0], ("logits_l2",))


def test_mark_modified_bumps_versions_and_drops_packed_filters():
    """the host side of showtell_amd.mark_modified: a write through .data leaves the version counter alone, mark_modified
    moves it for every parameter and buffer of a module (or for single tensors) and drops a backbone's packed filters"""
    from showtell_amd import mark_modified
    from showtell_amd.cnn import ResNet
    m = ResNet(18, 64)
    m._bb.packed, m._bb.packed_key = torch.zeros(1), ("stale",)
    tensors = dict(list(m.named_parameters()) + list(m.named_buffers()))
    before = {k: t._version for k, t in tensors.items()}
    m.linear_secondlast_layer.weight.data.normal_()
    m.model[0].weight.data.mul_(2.0)
    assert {k: t._version for k, t in tensors.items()} == before
    mark_modified(m)
    assert all(t._version > before[k] for k, t in tensors.items())
    assert m._bb.packed is None and m._bb.packed_key is None
    p, b = torch.nn.Parameter(torch.zeros(3)), torch.zeros(2)
    mark_modified(p, b)
    assert p._version == 1 and b._version == 1
    mark_modified([p, [b]], (t for t in (p,)), torch.zeros(0))
    assert p._version == 3 and b._version == 2
    with pytest.raises(TypeError):
        mark_modified("rnn")
    with pytest.raises(TypeError):
        mark_modified(3)


if __name__ == "__main__":
    for c in decoder_cases():
        print("decoder", c, {k: round(v, 1) for k, v in decoder_power(*c).items()})
    for c in encoder_cases():
        print("encoder eval", c, {k: round(v, 1) for k, v in encoder_power(*c).items()})
    print("encoder train", {k: round(v, 1) for k, v in encoder_power("seed", None, train=True).items()})
    print("encoder attn", {k: round(v, 1) for k, v in encoder_power("seed", None, attn=True).items()})
    for f in FAMILIES:
        for kind in sorted(P3_HYPER):
            steps, total, losses = trajectory_power(f, kind)
            print("trajectory", f, kind, "losses", [round(v, 2) for v in losses], "per step", [{k: round(v, 1) for k, v in m.items()} for m in steps],
                  "all steps", {k: round(v, 1) for k, v in total.items()})
