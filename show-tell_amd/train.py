"""The training step of the reference (main.py:136-152) on MI355X, plus a synthetic-data driver.

    optimizer.zero_grad(); feat = cnn(image); loss = CE(rnn(feat, cap, lens), packed(cap));
    loss.backward(); optimizer.step()

`Trainer.step` performs exactly that arithmetic, ordered so that data-parallel communication
hides behind the frozen backbone:  the previous step's gradient all-reduce and optimizer
update are completed AFTER this step's backbone forward (which reads only frozen weights,
cnn.py:47) and BEFORE its trainable part.  With one GPU the order is irrelevant and the result
is identical to the reference loop; `flush()` applies the last pending update.

Software pipelining across steps (`step(..., upcoming=[next images])`): because the backbone is frozen, the
forward of a LATER minibatch depends on nothing this step computes.  When the caller hands the next images over (a data
loader always has them), their backbone forwards are issued on side HIP streams (up to three in flight) and run beside this step's head /
decoder / backward (launch-bound wavefront, few-tile GEMMs) AND beside each other: two backbone forwards in flight fill
each other's launch tails and pair the HBM-bound normalise passes with the MFMA-bound convolutions (6.8 -> 5.5 ms per
forward measured, tools/two_stream_encoder.py).  The arithmetic and its order per sample are unchanged -- the running
BatchNorm buffers are updated in minibatch order (cnn.py) -- only the schedule is.
"""
import math
import os

import numpy as np
import torch

from .head import linear_bn1d
from .parallel import GradAllReducer, broadcast_state
from .rnn import check_label_smoothing, check_probability, sample_lengths


def synthetic_batch(B, V, seed=1, device="cuda", image_size=224, mean=12.5, std=2.5, lo=6, hi=25):
    """COCO-shaped synthetic minibatch in the layout utils.create_batch produces (utils.py:61-77):
    images (B,3,224,224) fp32, captions LongTensor (B,Tmax) zero padded, lengths sorted descending,
    tokens [<start>=1] + randint(4,V) + [<end>=2] (vocab_builder.py:66-69).  SURVEY 8(d)."""
    rng = np.random.RandomState(seed)
    lens = np.clip(np.rint(rng.normal(mean, std, size=B)), lo, hi).astype(np.int64)
    lens = np.sort(lens)[::-1].copy()
    cap = np.zeros((B, int(lens[0])), dtype=np.int64)
    for b, l in enumerate(lens):
        cap[b, 0] = 1
        cap[b, 1:l - 1] = rng.randint(4, V, size=l - 2)
        cap[b, l - 1] = 2
    g = torch.Generator(device="cpu").manual_seed(seed)
    images = torch.randn(B, 3, image_size, image_size, generator=g)
    return images.to(device), torch.from_numpy(cap).to(device), [int(l) for l in lens]


def self_critical_advantage(reward, baseline, greedy_reward=None):
    """reward (B, S) -> advantage (B, S).  'greedy': reward - the greedy caption's reward (B,) of the same image (self-critical
    sequence training); 'mean': reward - the mean reward of the image's OTHER samples (needs S >= 2).  Computed in float64 and
    returned as float32: equal rewards give an advantage of exactly 0."""
    reward = torch.as_tensor(reward).double()
    if reward.dim() != 2:
        raise ValueError(f"reward_fn must return (B, S) rewards (got shape {tuple(reward.shape)})")
    if baseline == "greedy":
        g = torch.as_tensor(greedy_reward).double().reshape(-1)
        if g.shape[0] != reward.shape[0]:
            raise ValueError(f"reward_fn must return one reward per greedy caption (got {g.shape[0]} for {reward.shape[0]} images)")
        return (reward - g[:, None]).float()
    if baseline == "mean":
        S = reward.shape[1]
        if S < 2:
            raise ValueError("baseline='mean' needs num_samples >= 2")
        return (reward - (reward.sum(1, keepdim=True) - reward) / (S - 1)).float()
    raise ValueError(f"baseline must be 'greedy' or 'mean' (got {baseline!r})")


def sample_caption_batch(ids, lengths):
    """The B * S sampled rows of ``sample`` as a caption batch: ids (B, S, T), lengths (B, S) -> (order, captions (B * S, T),
    lens list), rows sorted by length, descending and stable (what pack_padded_sequence asks for).  order[k] = b * S + s is the
    sample behind sorted row k: its image is order[k] // S, and a per-sample value v (B, S) goes along as v.reshape(-1)[order]."""
    B, S, T = ids.shape
    flat_len = lengths.reshape(B * S)
    order = torch.sort(flat_len, descending=True, stable=True)[1]
    return order, ids.reshape(B * S, T)[order].contiguous(), [int(l) for l in flat_len[order].tolist()]


def dropout_rank():
    """This process's rank among the data-parallel replicas (0 without torch.distributed)."""
    import torch.distributed as dist
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def linear_ss_schedule(start, end, steps):
    """The linear decay of Bengio et al. (2015) as a scheduled-sampling rate: p(i) = start + (end - start) * min(i, steps) / steps for
    the i-th `Trainer.step` (the paper decays the teacher-forcing probability 1 - p; a rate that rises from 0 is start < end)."""
    start, end = check_probability(start, "start"), check_probability(end, "end")
    if int(steps) != steps or steps < 1:
        raise ValueError(f"steps must be an integer >= 1 (got {steps!r})")
    return lambda i: start + (end - start) * min(max(int(i), 0), steps) / steps


def inverse_sigmoid_ss_schedule(k):
    """The inverse-sigmoid decay of Bengio et al. (2015): the teacher-forcing probability is k / (k + exp(i / k)), k >= 1, so the
    scheduled-sampling rate of the i-th `Trainer.step` is p(i) = 1 - k / (k + exp(i / k)): 1 / (k + 1) at i = 0, towards 1."""
    k = float(k)
    if not k >= 1.0:
        raise ValueError(f"k must be >= 1 (got {k!r})")

    def rate(i):
        x = max(int(i), 0) / k
        return 1.0 if x > 700.0 else 1.0 - k / (k + math.exp(x))
    return rate


class Trainer:
    def __init__(self, cnn, rnn, optimizer, world_size=1, label_smoothing=0.0, scheduled_sampling=0.0, ss_temperature=1.0, ss_top_k=0,
                 ss_generator=None):
        """`label_smoothing` in [0, 1): `step` trains on CrossEntropyLoss(label_smoothing=..) (``rnn.loss(.., label_smoothing=)``);
        0 is the reference's plain cross entropy.
        Dropout is the decoder's own (``RNN(.., dropout=, dropout_in=, dropout_out=)``, active in ``rnn.train()``): `step` and the
        loss half of `step_self_critical` draw one step of its masks each; the sampling half of `step_self_critical` (``sample``,
        ``sentence_index``) always runs the deterministic model.  The decoder of rank r (0 without torch.distributed) is re-seeded
        with its seed + r here, which also zeroes its step counter, so that data-parallel replicas draw different masks.
        `scheduled_sampling`: a rate p in [0, 1], or a callable that gets the count of earlier `step` calls (0, 1, ..) and returns
        it (`linear_ss_schedule`, `inverse_sigmoid_ss_schedule`).  With p > 0 `step` first rolls the deterministic decoder along
        the caption (``rnn.scheduled_inputs(.., p, ss_temperature, ss_top_k, ss_generator)``, no dropout) and trains on the mixed
        inputs; p = 0 is the step it was.  `step_self_critical` is unaffected."""
        self.label_smoothing = check_label_smoothing(label_smoothing)
        self.scheduled_sampling = scheduled_sampling if callable(scheduled_sampling) else check_probability(scheduled_sampling,
                                                                                                            "scheduled_sampling")
        self.ss_temperature, self.ss_top_k, self.ss_generator = ss_temperature, ss_top_k, ss_generator
        self.steps = 0        # `step` calls so far: what a scheduled-sampling schedule is asked with
        self.cnn, self.rnn, self.opt = cnn, rnn, optimizer
        self.reducer = GradAllReducer(world_size)
        if world_size > 1:
            broadcast_state([cnn, rnn], optimizer)         # replicas start from rank 0's weights and BN buffers
        if hasattr(rnn, "seed_dropout"):                   # data-parallel replicas draw different dropout masks: rank r gets seed + r
            rnn.seed_dropout(rnn.dropout_seed + dropout_rank())
        self.pending = False
        optimizer._pending_owner = self                    # optimizer.state_dict() / utils.create_checkpoint flush the deferred step
        self._pre = []        # FIFO of (images, pooled features, event, undo): backbone forwards issued ahead on the side streams
        self._side = []
        self._rr = 0
        self.depth = int(os.environ.get("ST_PIPE_DEPTH", "3"))        # backbone forwards kept in flight ahead of the trainable part (B=128 step: depth 1: 6.8 ms per forward, 2: 5.6, 3: 5.3 = 5.96 ms/step; 4: 6.35 ms/step, 5: 7.46 -- more forwards in flight evict each other's activations from the 256 MB Infinity Cache)

    def trainable_params(cnn, rnn):
        """main.py:96: rnn.parameters() + cnn.linear_secondlast_layer + cnn.last_layer."""
        return list(rnn.parameters()) + list(cnn.linear_secondlast_layer.parameters()) + list(cnn.last_layer.parameters())
    trainable_params = staticmethod(trainable_params)

    def _apply_pending(self):
        if self.pending:
            self.opt.grad_scale = self.reducer.finish()
            self.opt.step()
            self.pending = False

    def _backbone(self, image):
        """Backbone features of `image` on the current stream; takes the result issued ahead by `_prefetch` if the oldest one in
        flight is this batch."""
        main = torch.cuda.current_stream()
        if self._pre and self._pre[0][0] is image:
            _, pooled, ev, _ = self._pre.pop(0)
            main.wait_event(ev)
            pooled.record_stream(main)
            return pooled
        self._drop(0)                                  # unexpected batch: drop what was prefetched
        return self.cnn.backbone_features(image)

    def _drop(self, j):
        """Forget the prefetched forwards from the j-th on.  Their momentum updates of the running BatchNorm buffers (and
        num_batches_tracked) were already issued: they are undone, so that the buffers follow only the minibatches trained on,
        in order.  The current stream is ordered behind the side streams."""
        main = torch.cuda.current_stream()
        for s_ in self._side:
            main.wait_stream(s_)
        self.cnn.restore_running([e[3] for e in self._pre[j:]])
        self._pre = self._pre[:j]

    def _prefetch(self, image):
        if not self._side:
            self._side = [torch.cuda.Stream() for _ in range(self.depth)]
        side = self._side[self._rr % len(self._side)]
        self._rr += 1
        side.wait_stream(torch.cuda.current_stream())  # after everything already queued on the main stream
        undo = []
        with torch.cuda.stream(side):
            pooled = self.cnn.backbone_features(image, undo=undo)
            ev = torch.cuda.Event()
            ev.record(side)
        self._pre.append((image, pooled, ev, undo))

    def _features(self, image, upcoming):
        """What every kind of step starts with: the frozen backbone (taken from or issued to the side streams), the previous
        step's deferred optimizer update, zero_grad, and the trainable head.  Returns the (B, E) image features."""
        cnn = self.cnn
        pooled = self._backbone(image)                 # frozen, detached (cnn.py:46-47): overlaps the all-reduce
        # keep up to `depth` later minibatches' frozen backbones in flight, beside this step's trainable part and each other
        upcoming = [im for im in list(upcoming)[:self.depth] if im is not None]
        for j, im in enumerate(upcoming):
            if j < len(self._pre):
                if self._pre[j][0] is not im:          # the caller changed its mind: start over from here
                    self._drop(j)
                    self._prefetch(im)
            else:
                self._prefetch(im)
        self._apply_pending()                          # previous step's optimizer.step() (main.py:152)
        self.opt.zero_grad()                           # main.py:146
        return linear_bn1d(pooled, cnn.linear_secondlast_layer, cnn.last_layer, cnn.training, cnn.compute_dtype)

    @property
    def grad_norm(self):
        """The optimizer's ``last_grad_norm``: a 0-d device tensor holding the global norm of the (rank-averaged) gradient that
        the last APPLIED optimizer step saw -- the deferred one runs inside the next `step` or `flush` -- or None for an
        optimizer without one.  Reading its value synchronises; the training loop itself never does."""
        return getattr(self.opt, "last_grad_norm", None)

    def step(self, image, caption, caption_len, upcoming=()):
        """One training step.  `upcoming`: the images of the next minibatches, in order (at most `depth` are used).
        Gradient clipping, weight decay and the non-finite guard are the optimizer's keywords (``max_grad_norm``,
        ``weight_decay``, ``skip_nonfinite``, optim.py): they act inside the deferred optimizer step, after the all-reduce, on
        the device, and need nothing here.  With scheduled sampling on (see __init__) the roll-in runs after the trainable head, on
        this step's features; the deferred optimizer step and `upcoming` work as without it."""
        ss = self.scheduled_sampling
        p = check_probability(ss(self.steps), "scheduled_sampling") if callable(ss) else ss
        self.steps += 1
        feat = self._features(image, upcoming)
        if p:
            loss = self.rnn.loss(feat, caption, caption_len, label_smoothing=self.label_smoothing, scheduled_sampling=p,
                                 ss_temperature=self.ss_temperature, ss_top_k=self.ss_top_k, ss_generator=self.ss_generator)
        elif self.label_smoothing:
            loss = self.rnn.loss(feat, caption, caption_len, label_smoothing=self.label_smoothing)
        else:
            loss = self.rnn.loss(feat, caption, caption_len)    # main.py:148-149
        loss.backward()                                # main.py:151
        self.reducer.start(self.opt.flat_grad)
        self.pending = True
        return loss

    def step_self_critical(self, image, reward_fn, num_samples=5, baseline="greedy", upcoming=(), generator=None, uniforms=None,
                           end_id=2):
        """One reward-weighted step on the model's own samples (REINFORCE with a baseline; baseline='greedy' is self-critical
        sequence training): `num_samples` captions per image are drawn on the device (temperature 1, whole vocabulary),
        `reward_fn(ids (B, S, T) int64, lengths (B, S) int64) -> (B, S)` scores them on the host (CPU tensors; e.g.
        ``evaluation.cider_reward``), and the loss is sum over the sampled tokens of (reward - baseline) * -log p(token) / N_tok:
        ``rnn.loss`` with ``sequence_weight`` on the samples as a caption batch, the image features repeated.  The baseline is
        the reward of the greedy caption of the same image ('greedy') or the mean reward of the image's other samples ('mean').
        Backward and the deferred all-reduce / optimizer schedule are those of `step`.  Returns (loss, mean reward of the samples).
        Signed, reward-scaled losses are where an optimizer built with ``max_grad_norm`` (and ``skip_nonfinite``) earns its keep.
        `generator` / `uniforms` fix the draws as in ``RNN.sample``.
        A `reward_fn` with an ``advantage`` method (``evaluation.cider_reward_device``) scores on the device instead: the ids stay
        there, rewards and advantages come from one launch, only the lengths are read back (`_self_critical_on_device`), and the
        mean reward returned is a device tensor.  A plain callable takes the host path above, unchanged.
        The Trainer's `label_smoothing` does not apply here: a reward-weighted log-likelihood of the model's own samples is not a
        target distribution to be smoothed, so this step stays unsmoothed."""
        if baseline not in ("greedy", "mean"):
            raise ValueError(f"baseline must be 'greedy' or 'mean' (got {baseline!r})")
        if baseline == "mean" and num_samples < 2:
            raise ValueError("baseline='mean' needs num_samples >= 2")
        rnn = self.rnn
        feat = self._features(image, upcoming)
        B, S = feat.shape[0], int(num_samples)
        if hasattr(reward_fn, "advantage"):
            return self._self_critical_on_device(feat, reward_fn, S, baseline, generator, uniforms, end_id)
        with torch.no_grad():
            ids, _, lengths = rnn.sample(feat, S, temperature=1.0, top_k=0, end_id=end_id, generator=generator, uniforms=uniforms)
            greedy = None
            if baseline == "greedy":
                gids = rnn.sentence_index(feat).reshape(B, 1, -1)
                greedy = reward_fn(gids.cpu(), sample_lengths(gids, end_id).cpu())
            ids_cpu, len_cpu = ids.cpu(), lengths.cpu()
        reward = torch.as_tensor(reward_fn(ids_cpu, len_cpu), dtype=torch.float32)
        if tuple(reward.shape) != (B, S):
            raise ValueError(f"reward_fn must return {(B, S)} rewards (got shape {tuple(reward.shape)})")
        advantage = self_critical_advantage(reward, baseline, greedy)
        order, cap, lens = sample_caption_batch(ids_cpu, len_cpu)
        dev = feat.device
        feat_rep = feat[(order // S).to(dev)]          # the image behind every sorted row
        loss = rnn.loss(feat_rep, cap.to(dev), lens, sequence_weight=advantage.reshape(-1)[order])
        loss.backward()
        self.reducer.start(self.opt.flat_grad)
        self.pending = True
        return loss, reward.mean()

    def _self_critical_on_device(self, feat, reward_fn, S, baseline, generator, uniforms, end_id):
        """`step_self_critical` from the features on, for a `reward_fn` that scores on the device
        (``evaluation.cider_reward_device``): the sampled ids never leave it.  Rewards and advantages come from one
        ``reward_fn.advantage`` launch; only `lengths` goes to the host, because the packed loss needs Python lengths and the stable
        length sort of `sample_caption_batch`; the samples, the features and the advantages are gathered by that order on the
        device.  The mean reward is returned as a 0-d device tensor."""
        rnn, B = self.rnn, feat.shape[0]
        with torch.no_grad():
            ids, _, lengths = rnn.sample(feat, S, temperature=1.0, top_k=0, end_id=end_id, generator=generator, uniforms=uniforms)
            gids = rnn.sentence_index(feat).reshape(B, -1) if baseline == "greedy" else None
            reward, advantage, _ = reward_fn.advantage(ids, lengths, baseline, gids, check_lengths=False)   # lengths are sample's own
            flat_len = lengths.reshape(B * S).cpu()
        order = torch.sort(flat_len, descending=True, stable=True)[1]             # as sample_caption_batch
        lens = [int(l) for l in flat_len[order].tolist()]
        order = order.to(feat.device)
        cap = ids.reshape(B * S, ids.shape[2])[order].contiguous()
        loss = rnn.loss(feat[order // S], cap, lens, sequence_weight=advantage.reshape(-1)[order])
        loss.backward()
        self.reducer.start(self.opt.flat_grad)
        self.pending = True
        return loss, reward.mean()

    def flush(self):
        self._apply_pending()
