"""Do the kernels' cached weight copies follow every weight update?

In bf16 no kernel reads a parameter: each reads a derived copy -- rnn.working_copy's per-parameter bf16 copy, the flat
optimizers' bf16 shadow, the backbone's packed and fragment-major filters (cnn._Backbone.pack_weights), the flat BatchNorm
arrays.  A stale copy gives no fault and no NaN, only the old weights' plausible numbers.  Every case here builds a bf16 model
on weights W0, runs it so that every copy is cached (one loss().backward(), one sentence_index; the encoder one forward),
changes the weights to W1 by the path under test, runs again and compares with the float64 oracle (oracle/restatement.py)
on the kernels' view of W1 (bf16 rounding of every matrix, fp32 of what is read live).  No GPU run is compared with another.
tests/test_weight_coherence_inputs.py holds the inputs and proves, on the host, that the oracle on W0 misses every bound by
20 x or more; each case asserts that again for the weights it ended up with.

Paths   P1 load_state_dict after a forward                 P2 the same under a flat optim.SGD (parameters stay views of opt.flat)
        P3 three optim.SGD(momentum) / optim.Adam steps, shadow_dtype bf16 and None, the masters followed in float64
        P4 three torch.optim.SGD steps                     P5 in place under no_grad: copy_, mul_(-1), nn.init.normal_
        P6 storage replaced: p.data = t; .cpu() -> write -> .cuda(); the same round trip under a flat optimizer, then a step
        P7 utils.load_checkpoint into live models          P8 Trainer: two pipelined steps and flush
        P9 writes through .data followed by showtell_amd.mark_modified
P1 and P5 also change ONE tensor at a time (every tensor with a working copy, one convolution of each packing, the head's
Linear): a path-level case cannot show that one particular copy went stale.

What is not checked, and why.  The attention decoders return no feature gradient: loss and logits only.  cnn.ResNet's head in
train mode on 2 images: BatchNorm1d over a batch of two is gamma * sign(z0 - z1) + beta, which no weight moves and any rounding
flips; train mode checks the pooled features.  P3 / P4 feed the float64 optimizer the gradients backward() left on the GPU
(Adam's m / sqrt(v) turns the sign of a near-zero gradient element into a full step: with the oracle's own gradients the
master check would measure bf16 gradient noise, which tests/test_gpu_rnn_bptt_fused.py bounds, not the optimizer).

Bounds: LOSS_REL, GRAD_L2, GRAD_MAX, ROW_L2 of tests/test_gpu_decoder_bench_shape.py; the encoder's bf16 bound of
tests/test_gpu_encoder.py.  MEASURED (MI355X), worst over all cases, bound after the "/":
  plain decoders      loss 5.4e-4 / 5e-3   logits rel L2 3.0e-3 / 1e-2   rel max 4.0e-3 / 4e-2   dfeat worst row 1.4e-2 / 3e-2
  attention decoders  loss 1.4e-3 / 5e-3   logits rel L2 8.1e-3 / 1e-2   rel max 1.6e-2 / 4e-2   (single "load" of unit.weight_ih_l1;
                      the float64 oracle itself moves these logits by 5e-3 .. 1.2e-2 under a 2^-9 relative perturbation of the weights)
  encoder             pooled, eval 6.5e-3, train 2.9e-2 / 6e-2   head 6.7e-3 / 6e-2   cnn_attn feature map 5.7e-3 / 6e-2
  fp32 masters after an optim.SGD / optim.Adam / torch.optim.SGD step, beyond one fp32 ulp: rel L2 and rel max 7.4e-6 / 1e-2, 4e-2
  bf16 working copies against bf16(master): bit-exact in every case
"""
import pytest
import torch
import torch.nn as nn

from tests import test_weight_coherence_inputs as I
from tests.test_gpu_decoder_bench_shape import _check_update

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
VOCAB = lambda w: {"<start>": 1}[w]


# ---- decoders ------------------------------------------------------------------------------------------------------------

def _new_decoder(family, params):
    from showtell_amd.rnn import RNN
    from showtell_amd.rnn_attn import RNN_Attn
    from showtell_amd.rnn_attn_LSTM import RNN_Attn as RNN_Attn_LSTM
    from showtell_amd.rnn_lstm import RNN as RNN_LSTM
    g, lstm = I.geometry(family), I.cell_of(family) == "lstm"
    if I.is_attn(family):
        m = (RNN_Attn_LSTM if lstm else RNN_Attn)(g["E"], g["F"], g["A"], g["H"], g["V"], g["L"], dtype=BF16)
    else:
        m = (RNN_LSTM if lstm else RNN)(g["E"], g["H"], g["V"], g["L"], dtype=BF16)
    m.load_state_dict({k: v.clone() for k, v in params.items()})
    return m.cuda().train()


def _loss(m, family, feat, cap, lens):
    return m.loss(feat, cap, lens, 1.0) if I.is_attn(family) else m.loss(feat, cap, lens)


def _warm(m, family):
    """every cache filled from the current weights: a training forward and backward, a greedy decode"""
    feat, cap, lens = I.decoder_batch(family)
    _loss(m, family, feat.cuda(), cap.cuda(), lens).backward()
    if I.is_attn(family):
        m.sentence_index(feat.cuda(), VOCAB)
    else:
        m.sentence_index(feat.cuda())
    torch.cuda.synchronize()


def _masters(m):
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


def _gpu_outputs(m, family, batch=0):
    """{loss, logits, dfeat} of one loss().backward() and one forward on the GPU, as float64 on the host"""
    feat, cap, lens = I.decoder_batch(family, batch)
    attn = I.is_attn(family)
    fd = feat.cuda().requires_grad_(not attn)
    loss = _loss(m, family, fd, cap.cuda(), lens)
    loss.backward()
    with torch.no_grad():
        out = m(feat.cuda(), cap.cuda(), lens)
    torch.cuda.synchronize()
    return dict(loss=loss.item(), logits=(out[0] if attn else out).double().cpu(), dfeat=None if attn else fd.grad.double().cpu())


def _check_working_copies(params, tag):
    """bit-exact and oracle-free: what the kernels read of every matrix is the bf16 rounding of what the parameter holds now"""
    from showtell_amd.rnn import working_copy
    for k, p in params:
        if p.dim() >= 2:
            assert torch.equal(working_copy(p, BF16), p.detach().bfloat16()), (tag, k, "stale bf16 working copy")


def _assert_moved(family, masters, tag, outputs, batch=0):
    """the power condition for the weights this case ended up with: the oracle on W0 misses the bounds by 20 x"""
    w0 = I.decoder_w0_oracle(family) if batch == 0 else I.decoder_oracle(family, I.decoder_params(family, 0), batch)
    e = I.decoder_errors(w0, I.decoder_oracle(family, masters, batch))
    for k, v in e.items():
        if outputs is None or k in outputs:
            assert v >= I.POWER * I.BOUNDS[k], (tag, k, "the oracle on W0 is within 20 x the bound of the oracle on W1", v)


def _check_decoder(m, family, masters, tag, batch=0):
    """the GPU's loss, logits and d loss / d feat against the float64 oracle on `masters`; then the working copies"""
    ref = I.decoder_oracle(family, masters, batch)
    errs = I.decoder_errors(_gpu_outputs(m, family, batch), ref)
    print(f"MEASURE {tag}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    _check_working_copies(m.named_parameters(), tag)
    for k, v in errs.items():
        assert v < I.BOUNDS[k], (tag, k, v, I.BOUNDS[k])


def _views_of_flat(opt):
    return all(p.data_ptr() == opt.flat.data_ptr() + 4 * o for p, o in zip(opt.params, opt.offsets))


def _write(m, w1, names, how, normal_scale=I.NORMAL_SCALE):
    """change the tensors `names` of the live module `m` to their values in `w1` by the path `how`"""
    named = dict(m.named_parameters())
    named.update(dict(m.named_buffers()))
    torch.manual_seed(1234)
    if how == "load":                                   # P1 / P2
        sd = _masters(m)
        sd.update({k: w1[k].clone() for k in names})
        m.load_state_dict(sd)
    elif how in ("copy", "neg", "normal"):              # P5
        with torch.no_grad():
            for k in names:
                if how == "copy":
                    named[k].copy_(w1[k].cuda())
                elif how == "neg":
                    named[k].mul_(-1)
                else:                                    # drawn on the device: W1 is read back from the masters
                    nn.init.normal_(named[k], 0.0, I.redraw_std(named[k].detach().cpu(), normal_scale))
    elif how == "data_assign":                          # P6
        for k in names:
            named[k].data = w1[k].cuda()
    elif how == "cpu_cuda":                             # P6: the write itself is invisible (.data), the move must not be
        m.cpu()
        named = dict(m.named_parameters())
        named.update(dict(m.named_buffers()))           # Module._apply replaces buffer objects
        for k in names:
            named[k].data.copy_(w1[k])
        m.cuda()
    elif how == "data_marked":                          # P9
        from showtell_amd import mark_modified
        for k in names:
            named[k].data.copy_(w1[k].cuda())
        mark_modified(m)
    else:
        raise ValueError(how)
    torch.cuda.synchronize()


def _float_names(params):
    return [k for k, v in params.items() if v.is_floating_point()]


WHOLE = {  # path -> (how, W1 as tests/test_weight_coherence_inputs.py names it, a flat optimizer attached first)
    "P1_load": ("load", "seed", False), "P2_load_flat_optimizer": ("load", "seed", True),
    "P5_copy": ("copy", "seed", False), "P5_neg": ("neg", "neg", False), "P5_normal": ("normal", "normal", False),
    "P6_data_assign": ("data_assign", "seed", False), "P6_cpu_cuda": ("cpu_cuda", "seed", False),
    "P9_data_marked": ("data_marked", "seed", False),
}


@pytest.mark.parametrize("path", sorted(WHOLE))
@pytest.mark.parametrize("family", I.FAMILIES)
def test_decoder_follows_a_whole_model_update(family, path):
    from showtell_amd import optim
    how, op, flat = WHOLE[path]
    m = _new_decoder(family, I.decoder_params(family, 0))
    opt = optim.SGD(list(m.parameters()), lr=0.5, momentum=0.9) if flat else None
    _warm(m, family)
    flat_ptr = opt.flat.data_ptr() if flat else None
    w1 = I.decoder_w1(family, op, None)
    _write(m, w1, _float_names(w1), how)
    if flat:                                            # before anything that could re-flatten: the write went INTO the flat buffer
        assert opt.flat.data_ptr() == flat_ptr and _views_of_flat(opt), "load_state_dict detached the parameters from opt.flat"
        for k, p in m.named_parameters():
            o = opt.offsets[[id(q) for q in opt.params].index(id(p))]
            assert torch.equal(opt.flat[o:o + p.numel()].cpu(), w1[k].reshape(-1)), (path, k)
    masters = _masters(m)
    if how != "normal":                                 # the masters hold W1 itself; nn.init.normal_ drew them on the device
        for k in w1:
            assert torch.equal(masters[k], w1[k]), (path, k)
    tag = f"{path} {family}"
    _assert_moved(family, masters, tag, I.decoder_powered(family, op, None, device_draw=True))
    _check_decoder(m, family, masters, tag)
    if flat:
        assert opt.flat.data_ptr() == flat_ptr and _views_of_flat(opt)


def _single_cases():
    return [(f, k) for f in I.FAMILIES for k in I.single_tensors(f)]


@pytest.mark.parametrize("how", I.OPS)
@pytest.mark.parametrize("family,name", _single_cases())
def test_decoder_follows_an_update_of_one_tensor(family, name, how):
    """P1 ("load") and P5 ("copy", "neg", "normal") on one tensor, everything else left at W0"""
    m = _new_decoder(family, I.decoder_params(family, 0))
    _warm(m, family)
    w1 = I.decoder_w1(family, how, name)
    _write(m, w1, [name], how)
    masters = _masters(m)
    for k in w1:
        if how != "normal" or k != name:
            assert torch.equal(masters[k], w1[k]), (how, k)
    tag = f"single {how} {family} {name}"
    _assert_moved(family, masters, tag, I.decoder_powered(family, how, name, device_draw=True))
    _check_decoder(m, family, masters, tag)


def _check_masters(named, fol, before, tag):
    """the GPU's fp32 masters after a step against the float64 follower's (tests/test_gpu_decoder_bench_shape.py:_check_update)"""
    for k, p in named:
        after = p.detach().double().cpu()
        if torch.equal(fol.p[k], before[k]):            # a tensor whose gradient is exactly zero does not move
            assert torch.equal(after, before[k]), (tag, k)
            continue
        _check_update(after, before[k], fol.p[k], f"{tag} master {k}")


def _train_steps(m, family, opt, kind, tag, steps=I.P3_STEPS, start=None):
    """`steps` training steps, step s on minibatch s.  Before each step the GPU's loss / logits / dfeat on that minibatch are
    checked against the oracle on the follower's weights (after the first step: the weights the previous step produced); the
    follower then takes the same step in float64 from the gradients that backward() left on the GPU, and the GPU's masters
    are checked against it.  The weights of the last step are checked on one more minibatch."""
    named = list(m.named_parameters())
    fol = I.Follower(kind, {k: v for k, v in (start or _masters(m)).items() if k in dict(named)})
    for s in range(steps):
        opt.zero_grad()
        _check_decoder(m, family, {**_masters(m), **fol.masters()}, f"{tag} before step {s + 1}", batch=s)     # leaves one backward's gradients
        grads = {k: p.grad.detach().double().cpu() for k, p in named}
        before = {k: v.clone() for k, v in fol.p.items()}
        fol.step(grads)
        opt.step()
        torch.cuda.synchronize()
        _check_masters(named, fol, before, f"{tag} step {s + 1}")
    final = {**_masters(m), **fol.masters()}
    _check_decoder(m, family, final, f"{tag} after step {steps}", batch=steps)
    return final


@pytest.mark.parametrize("shadow", ["bf16", "none"])
@pytest.mark.parametrize("kind", ["sgd", "adam"])
@pytest.mark.parametrize("family", I.FAMILIES)
def test_decoder_follows_flat_optimizer_steps(family, kind, shadow):
    """P3.  shadow_dtype=None over a bf16 model: the optimizer owns no bf16 copy, the kernels read rnn.working_copy's, which
    must notice that the step kernel wrote the masters through a raw pointer."""
    from showtell_amd import optim
    m = _new_decoder(family, I.decoder_params(family, 0))
    sd = BF16 if shadow == "bf16" else None
    opt = (optim.SGD if kind == "sgd" else optim.Adam)(list(m.parameters()), **I.P3_HYPER[kind], shadow_dtype=sd)
    _warm(m, family)
    tag = f"P3 {kind} shadow={shadow} {family}"
    final = _train_steps(m, family, opt, kind, tag)
    _assert_moved(family, final, tag, ("logits_l2",), batch=I.P3_STEPS)
    assert _views_of_flat(opt)


@pytest.mark.parametrize("family", I.FAMILIES)
def test_decoder_follows_torch_optim_sgd_steps(family):
    """P4: INTEGRATION.md's "torch.optim.SGD also works", over a bf16 model's GPU parameters"""
    m = _new_decoder(family, I.decoder_params(family, 0))
    opt = torch.optim.SGD(m.parameters(), **I.P3_HYPER["sgd"])
    _warm(m, family)
    tag = f"P4 torch.optim.SGD {family}"
    final = _train_steps(m, family, opt, "sgd", tag)
    _assert_moved(family, final, tag, ("logits_l2",), batch=I.P3_STEPS)


@pytest.mark.parametrize("family", I.FAMILIES)
def test_decoder_and_flat_optimizer_survive_a_cpu_round_trip(family):
    """P6: .cpu() / .cuda() replaces every parameter's storage under a live flat optimizer; the weights written in between
    must be what the kernels read, and the next opt.step() must move the weights the kernels read"""
    from showtell_amd import optim
    m = _new_decoder(family, I.decoder_params(family, 0))
    opt = optim.SGD(list(m.parameters()), **I.P3_HYPER["sgd"])
    _warm(m, family)
    w1 = I.decoder_params(family, 1)
    _write(m, w1, _float_names(w1), "cpu_cuda")
    tag = f"P6 round trip under optim.SGD {family}"
    _check_decoder(m, family, w1, tag)
    final = _train_steps(m, family, opt, "sgd", tag, steps=1, start=w1)
    assert _views_of_flat(opt)
    e = I.decoder_errors(I.decoder_oracle(family, w1, 1), I.decoder_oracle(family, final, 1))
    assert e["logits_l2"] >= I.POWER * I.BOUNDS["logits_l2"], (tag, "the step moved the logits too little to be seen", e)


# ---- encoder -------------------------------------------------------------------------------------------------------------

def _new_encoder(params, attn=False, train=False):
    from showtell_amd.cnn import ResNet
    from showtell_amd.cnn_attn import ResNet as ResNetAttn
    m = (ResNetAttn if attn else ResNet)(I.ENC_VERSION, I.ENC_EMBED, dtype=BF16)
    m.load_state_dict({k: v.clone() for k, v in params.items()})
    return m.cuda().train(train)


def _encoder_outputs(m, attn, train, batch=0):
    x = I.encoder_images(batch).cuda()
    with torch.no_grad():
        if attn:
            out = {"map": m(x)}
        elif train:
            out = {"pooled": m.backbone_features(x)}          # the head on a batch of two: see the module docstring
        else:
            out = {"pooled": m.backbone_features(x), "head": m(x)}
    torch.cuda.synchronize()
    return {k: v.detach().double().cpu() for k, v in out.items()}


def _check_encoder(m, masters, tag, attn=False, train=False, outputs=None):
    ref = I.encoder_oracle(masters, train, attn)
    got = _encoder_outputs(m, attn, train)
    errs = {k: I.enc_rel(got[k], ref[k]) for k in got}
    w0 = I.encoder_w0_oracle(train, attn)
    for k in errs:
        if outputs is None or k in outputs:
            gap = I.enc_rel(w0[k], ref[k])
            assert gap >= I.POWER * I.BOUNDS[k], (tag, k, "the oracle on W0 is within 20 x the bound of the oracle on W1", gap)
    print(f"MEASURE {tag}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < I.BOUNDS[k], (tag, k, v, I.BOUNDS[k])


ENC_WHOLE = {"P1_load": "load", "P5_copy": "copy", "P6_data_assign": "data_assign", "P6_cpu_cuda": "cpu_cuda",
             "P9_data_marked": "data_marked"}


@pytest.mark.parametrize("path", sorted(ENC_WHOLE))
def test_encoder_follows_a_whole_model_update(path):
    m = _new_encoder(I.encoder_params(0))
    _encoder_outputs(m, False, False)
    w1 = I.encoder_params(1)
    _write(m, w1, _float_names(w1), ENC_WHOLE[path])
    masters = _masters(m)
    for k in _float_names(w1):
        assert torch.equal(masters[k], w1[k]), (path, k)
    _check_encoder(m, masters, f"{path} cnn eval")


@pytest.mark.parametrize("how", ["load", "cpu_cuda"])
def test_encoder_train_mode_follows_an_update(how):
    """train-mode BatchNorm; "cpu_cuda" goes through ResNet._apply with the running buffers a forward has already updated"""
    m = _new_encoder(I.encoder_params(0, damp=True), train=True)
    _encoder_outputs(m, False, True)
    w1 = I.encoder_params(1, damp=True)
    _write(m, w1, _float_names(w1), how)
    _check_encoder(m, w1, f"{how} cnn train", train=True)


@pytest.mark.parametrize("how", ["load", "data_marked", "cpu_cuda"])
def test_attention_encoder_follows_an_update(how):
    m = _new_encoder(I.encoder_params(0), attn=True)
    _encoder_outputs(m, True, False)
    w1 = I.encoder_params(1)
    _write(m, w1, _float_names(w1), how)
    _check_encoder(m, w1, f"{how} cnn_attn eval", attn=True)


@pytest.mark.parametrize("how,key", [c for c in I.encoder_cases() if c[0] != "seed"])
def test_encoder_follows_an_update_of_one_tensor(how, key):
    """P1 / P5 on one convolution of each packing and on the head's Linear; nn.init.normal_ also on every convolution and the
    head at once; and (load_state_dict only) every BatchNorm2d gain and running variance: those are read live from the flat
    arrays, which load_state_dict writes in place"""
    m = _new_encoder(I.encoder_params(0))
    _encoder_outputs(m, False, False)
    bb = m._bb
    if key in I.ENC_CONVS:                               # the case really is the packing its name says
        idx, name = I.ENC_CONVS[key]
        inf, conv = bb.info[idx], dict(m.named_parameters())[name]
        assert bb.pairs[idx][0].weight is conv
        frag = {"stem7x7": (7, False), "c3x3_frag": (3, True), "c3x3_frag_l3": (3, True), "c3x3_s2": (3, False), "down1x1": (1, None)}[key]
        assert inf["k"] == frag[0] and (frag[1] is None or (inf["ntw"] > 0) == frag[1]), (key, inf)
    w1 = I.encoder_w1(how, key)
    w0 = I.encoder_params(0)
    names = [k for k in _float_names(w1) if not torch.equal(w1[k], w0[k])]
    assert names and (key == I.ENC_BN or sorted(names) == sorted(I.encoder_names(key)))
    if key == I.ENC_BN:
        flat_ptr = bb.flat["gamma"].data_ptr()
    _write(m, w1, names, how, normal_scale=I.ENC_SHRINK)
    masters = _masters(m)
    for k in _float_names(w1):                           # nn.init.normal_ drew on the device: W1 is what the masters hold
        if how != "normal" or k not in names:
            assert torch.equal(masters[k], w1[k]), (how, key, k)
        else:
            assert not torch.equal(masters[k], w0[k]), (how, key, k)
    if key == I.ENC_BN:                                  # still the same flat arrays, read live: nothing was re-built
        assert bb.flat["gamma"].data_ptr() == flat_ptr and bb._bn_ok(torch.device("cuda", torch.cuda.current_device()))
    _check_encoder(m, masters, f"single {how} cnn {key}", outputs=("head",) if key == "head" else None)


# ---- whole pipelines -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", ["gru", "lstm"])
def test_load_checkpoint_into_live_models(family, tmp_path):
    """P7: evaluation.test_model's loop over several checkpoints -- utils.load_checkpoint(path, cnn, rnn, opt) into models that
    have already run.  The checkpoint is written by utils.create_checkpoint from a second set of weights."""
    from showtell_amd import optim, utils
    from showtell_amd.cnn import ResNet
    from showtell_amd.train import Trainer
    cnn = _new_encoder(I.encoder_params(0))
    rnn = _new_decoder(family, I.decoder_params(family, 0))
    opt = optim.SGD(Trainer.trainable_params(cnn, rnn), **I.P3_HYPER["sgd"])
    _encoder_outputs(cnn, False, False)
    _warm(rnn, family)
    # the second set: host modules that never ran
    enc1, dec1 = I.encoder_params(1), I.decoder_params(family, 1)
    cnn1 = ResNet(I.ENC_VERSION, I.ENC_EMBED, dtype=BF16)
    cnn1.load_state_dict(enc1)
    rnn1 = type(rnn)(*[I.geometry(family)[k] for k in ("E", "H", "V", "L")], dtype=BF16)
    rnn1.load_state_dict(dec1)
    opt1 = optim.SGD(Trainer.trainable_params(cnn1, rnn1), **I.P3_HYPER["sgd"])
    path = utils.create_checkpoint(cnn1, rnn1, opt1, 3, 7, [1.0], {"output_dir": str(tmp_path)})
    flat_ptr = opt.flat.data_ptr()
    assert utils.load_checkpoint(path, cnn, rnn, opt) == (3, 7)
    # had load_state_dict detached a parameter, optimizer.load_state_dict (-> _ensure_flat) would have built a new flat buffer
    assert opt.flat.data_ptr() == flat_ptr and _views_of_flat(opt), "load_checkpoint detached the parameters from opt.flat"
    _check_encoder(cnn, enc1, f"P7 load_checkpoint cnn ({family})")
    _assert_moved(family, dec1, "P7", None)
    _check_decoder(rnn, family, dec1, f"P7 load_checkpoint {family}")


@pytest.mark.parametrize("family", ["gru", "lstm"])
def test_trainer_steps_leave_coherent_copies(family):
    """P8: two Trainer steps, the first with the next images handed over (their backbone forward runs ahead on a side stream,
    the optimizer step is deferred behind the next backbone forward), then flush()"""
    from showtell_amd import optim
    from showtell_amd.train import Trainer
    cnn = _new_encoder(I.encoder_params(0), train=True)
    rnn = _new_decoder(family, I.decoder_params(family, 0))
    trainable = Trainer.trainable_params(cnn, rnn)
    opt = optim.SGD(trainable, **I.P3_HYPER["sgd"])
    _warm(rnn, family)
    B = len(I.geometry(family)["lens"])
    images = [torch.randn(B, 3, 64, 64, generator=torch.Generator().manual_seed(300 + i)).cuda() for i in range(2)]
    tr = Trainer(cnn, rnn, opt)
    for i in range(2):
        _, cap, lens = I.decoder_batch(family, i)
        tr.step(images[i], cap.cuda(), lens, upcoming=[images[1]] if i == 0 else ())
    tr.flush()
    torch.cuda.synchronize()
    tag = f"P8 Trainer {family}"
    head = [(f"cnn.{k}", p) for k, p in cnn.named_parameters() if any(p is q for q in trainable)]
    _check_working_copies(list(rnn.named_parameters()) + head, tag)
    masters = _masters(rnn)
    _assert_moved(family, masters, tag, ("logits_l2",), batch=2)
    _check_decoder(rnn, family, masters, tag, batch=2)
