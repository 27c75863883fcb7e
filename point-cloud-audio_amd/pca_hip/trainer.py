"""Train / eval engine for the ST classifier on MI355X.

Replaces the training loop of Code/settransformer.py:96-112 (and settransformertemp.py):
``DataLoader -> .to(device) -> nn.DataParallel(model)(imgs) -> CrossEntropyLoss -> backward ->
Adam.step -> .item()`` becomes, per step and per GPU,

    [pack batch] -> pca_st_train_fwd_bwd -> all-reduce(gradients) -> pca_adam_step

or, with ``overlap`` (large models: the exchange hides under the rest of the backward),

    [pack batch] -> pca_st_train_fwd_bwd(phase 0) -> all-reduce(bucket enc.1+dec)
                 -> pca_st_train_fwd_bwd(phase 1) -> all-reduce(bucket enc.0) -> pca_adam_step

* one process per GPU; parameters, gradients and Adam moments are flat fp32 vectors in
  state_dict order, so the all-reduce is over two contiguous buckets and the optimiser is
  one fused kernel; the nn.Module's parameters are views of the flat vector;
* the device work of a step is captured once into hipGraphs (torch.cuda.CUDAGraph) and
  replayed, so no Python / autograd / allocator work sits between kernels;
* nn.DataParallel (Code/settransformer.py:94: single process, per-step parameter broadcast,
  scatter and gather) is replaced by an RCCL all-reduce of gradients (torch.distributed
  backend 'nccl' over xGMI): one message between the backward and the optimiser, or two
  buckets with the first on a side stream under the enc.0 backward (``overlap``);
* loss / accuracy are accumulated on the device and read once per epoch instead of the
  two ``.item()`` host syncs per step of Code/settransformer.py:110-112.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Optional, Tuple

import torch
import torch.distributed as dist

from . import _lib
from ._lib import StConfig, check, lib
from .ops import _need_cuda


def st_config(model, B: int, N: int, mode: int = _lib.MODE_F32) -> StConfig:
    """Read the architecture off an ``models.ST`` instance (bare, or wrapped in
    ``nn.DataParallel`` as ``runfiles.load_run`` / Code/pceval.py:46 hand it over)."""
    model = getattr(model, "module", model)
    isab0 = model.enc[0]
    if getattr(isab0.mab0, "ln0", None) is not None:
        raise _lib.PcaHipError("the whole-model engine covers ST(ln=False) (45 tensors); a model "
                               "with LayerNorms runs through the nn.Module path")
    d = isab0.mab0.dim_V
    return StConfig(B, N, isab0.mab1.fc_q.in_features, d, isab0.mab0.num_heads,
                    isab0.I.shape[1], model.dec[0].S.shape[1],
                    model.dec[1].out_features, mode)


def flatten_parameters(model) -> torch.Tensor:
    """Re-home every parameter of ``model`` as a view of ONE flat fp32 vector (state_dict
    order, the layout pca_st_* expects) and return that vector.  Idempotent: a model that
    is already flat keeps its vector (so several engines can share one model)."""
    model = getattr(model, "module", model)
    params = list(model.parameters())
    names = [n for n, _ in model.named_parameters()]
    assert names == list(model.state_dict().keys()), "unexpected parameter order"
    flat = getattr(model, "_pca_flat", None)
    if flat is not None:
        off, ok = 0, True
        for p in params:
            ok = ok and p.data_ptr() == flat.data_ptr() + 4 * off and p.is_contiguous()
            off += p.numel()
        if ok and off == flat.numel():
            return flat
    flat = torch.cat([p.detach().reshape(-1).float() for p in params]).contiguous()
    off = 0
    for p in params:
        n = p.numel()
        p.data = flat[off:off + n].view_as(p)
        off += n
    object.__setattr__(model, "_pca_flat", flat)
    return flat


class ShardedIndexStream:
    """Per-rank stream of set indices with DistributedSampler semantics: one
    seeded permutation per epoch, shared by all ranks; rank r takes elements r::world of it
    (the tail that does not divide evenly is dropped so that every rank runs the same number
    of steps).  Pure index logic: works on any device, tested on CPU with gloo."""

    def __init__(self, n: int, batch: int, rank: int = 0, world: int = 1, seed: int = 0,
                 shuffle: bool = True, device="cpu"):
        self.n, self.B, self.rank, self.world = int(n), int(batch), rank, world
        self.seed, self.shuffle, self.device = seed, shuffle, device
        self.epoch = 0
        self._perm = None
        self._cursor = 0
        if self.n // self.world < self.B:
            raise ValueError(f"dataset of {n} sets is too small for batch {batch} x {world} ranks")

    def per_rank(self) -> int:
        return self.n // self.world

    def _share(self, epoch: int) -> torch.Tensor:
        """This rank's share of the permutation of ``epoch``: a function of (seed, epoch) alone."""
        per = self.per_rank()
        if self.shuffle:
            g = torch.Generator(device="cpu").manual_seed(self.seed + epoch)
            perm = torch.randperm(self.n, generator=g)
        else:
            perm = torch.arange(self.n)
        return perm[self.rank:per * self.world:self.world].contiguous().to(self.device)

    def state(self) -> dict:
        """(seed, epoch, cursor): all it takes to hand out the remaining batches again."""
        return dict(seed=int(self.seed), epoch=int(self.epoch), cursor=int(self._cursor))

    def load_state(self, state: dict) -> None:
        """Continue where ``state()`` was taken; the current permutation is re-derived, not stored."""
        self.seed, self.epoch = int(state["seed"]), int(state["epoch"])
        self._cursor = int(state["cursor"])
        self._perm = self._share(self.epoch - 1) if self.epoch > 0 else None

    def next(self) -> torch.Tensor:
        per = self.per_rank()
        if self._perm is None or self._cursor + self.B > per:
            self._perm = self._share(self.epoch)
            self._cursor = 0
            self.epoch += 1
        out = self._perm[self._cursor:self._cursor + self.B]
        self._cursor += self.B
        return out

    def steps_per_epoch(self) -> int:
        return self.per_rank() // self.B

    def next_epoch(self) -> torch.Tensor:
        """All index batches of this rank's next epoch back to back ([steps_per_epoch * B]) -
        the same sequence ``next()`` would hand out one batch at a time."""
        spe = self.steps_per_epoch()
        first = self.next()
        # ``next`` has just started an epoch (it only does so with the cursor at 0)
        assert self._cursor == self.B
        self._cursor = spe * self.B
        return torch.cat([first, self._perm[self.B:spe * self.B]]) if spe > 1 else first


def allreduce_buckets(grads: torch.Tensor, split: int, group=None, first_stream=None):
    """Sum the flat gradient vector over the ranks in the two buckets of SURVEY.md 8e:
    [split, end) (enc.1 + dec, complete after backward phase 0) and [0, split) (enc.0).
    With ``first_stream`` the first bucket is reduced on that (side) stream so that it overlaps
    the remaining backward; the caller joins the streams before the optimiser."""
    if first_stream is not None:
        with torch.cuda.stream(first_stream):
            dist.all_reduce(grads[split:], group=group)
    else:
        dist.all_reduce(grads[split:], group=group)
    return lambda: dist.all_reduce(grads[:split], group=group)


def warmup_cosine(base_lr: float, warmup_steps: int, total_steps: int,
                  lr_min: float = 0.0) -> list:
    """The learning rate of steps 1 .. total_steps as a list (``Trainer(lr_schedule=)``), in float64:
    a linear ramp base_lr * t / warmup_steps over the first ``warmup_steps`` steps (so it starts at
    base_lr / warmup_steps), then half a cosine from base_lr down to ``lr_min`` at the last step."""
    warmup_steps, total_steps = int(warmup_steps), int(total_steps)
    if not 0 <= warmup_steps <= total_steps or total_steps < 1:
        raise ValueError(f"warmup_cosine: warmup_steps={warmup_steps} total_steps={total_steps}")
    table = []
    for t in range(1, total_steps + 1):
        if t <= warmup_steps:
            table.append(float(base_lr) * t / warmup_steps)
        else:
            frac = (t - warmup_steps) / max(1, total_steps - warmup_steps)
            table.append(float(lr_min) + 0.5 * (float(base_lr) - float(lr_min))
                         * (1.0 + math.cos(math.pi * frac)))
    return table


def _lr_table(lr_schedule, schedule_steps) -> Optional[torch.Tensor]:
    """``lr_schedule`` (a sequence of floats, or a callable step -> lr with ``schedule_steps``; steps
    count from 1) as a CPU fp32 vector, or None."""
    if lr_schedule is None:
        if schedule_steps is not None:
            raise ValueError("schedule_steps without lr_schedule")
        return None
    if callable(lr_schedule):
        if schedule_steps is None or int(schedule_steps) < 1:
            raise ValueError("a callable lr_schedule needs schedule_steps >= 1")
        values = [float(lr_schedule(t)) for t in range(1, int(schedule_steps) + 1)]
    else:
        values = [float(x) for x in lr_schedule]
        if schedule_steps is not None and int(schedule_steps) != len(values):
            raise ValueError(f"schedule_steps={schedule_steps} but lr_schedule has {len(values)} entries")
    if not values:
        raise ValueError("lr_schedule is empty")
    table = torch.tensor(values, dtype=torch.float64).to(torch.float32)
    if not bool(torch.isfinite(table).all()):
        raise ValueError("lr_schedule holds a non-finite learning rate")
    return table


def no_decay_groups() -> list:
    """The usual ``Trainer(param_groups=)`` preset: no weight decay on the biases, on the inducing
    points ``enc.*.I`` and on the seed ``dec.0.S``; every rate multiplier 1."""
    return [(r"\.bias$", 1.0, 0.0), (r"\.I$", 1.0, 0.0), (r"\.S$", 1.0, 0.0)]


def resolve_param_groups(model, param_groups) -> dict:
    """``param_groups``, a sequence of (regex, lr_scale, wd_scale), against the state_dict keys of
    ``model`` (``re.search``; the first match wins, an unmatched tensor gets (1, 1)) as segments of the
    flat parameter vector: adjacent tensors with equal scales are one segment.  Returns ``seg_end``
    (ascending ints, the last is the parameter count), ``lr_scale`` and ``wd_scale`` (one float per
    segment) and ``tensors`` ({key: (lr_scale, wd_scale)}).  A pattern that matches no tensor raises
    and names the pattern."""
    import re
    model = getattr(model, "module", model)
    groups = [(str(pat), float(ls), float(ws)) for pat, ls, ws in param_groups]
    for pat, ls, ws in groups:
        if not (math.isfinite(ls) and math.isfinite(ws)) or ls < 0.0 or ws < 0.0:
            raise ValueError(f"param_groups: {pat!r} has lr_scale={ls}, wd_scale={ws}; both must be "
                             "finite and >= 0")
    used = [False] * len(groups)
    tensors, seg_end, lr_scale, wd_scale = {}, [], [], []
    off = 0
    for key, p in model.state_dict().items():
        scales = (1.0, 1.0)
        for gi, (pat, ls, ws) in enumerate(groups):
            if re.search(pat, key):
                scales = (ls, ws)
                used[gi] = True
                break
        tensors[key] = scales
        off += p.numel()
        if seg_end and (lr_scale[-1], wd_scale[-1]) == scales:
            seg_end[-1] = off
        elif p.numel():
            seg_end.append(off)
            lr_scale.append(scales[0])
            wd_scale.append(scales[1])
    # a pattern shadowed by an earlier one still counts as matching if it matches a key at all
    for gi, (pat, _, _) in enumerate(groups):
        if not used[gi] and not any(re.search(pat, k) for k in tensors):
            raise ValueError(f"param_groups: the pattern {pat!r} matches no tensor of the model")
    if len(seg_end) > 256:
        raise ValueError(f"param_groups resolve to {len(seg_end)} segments; pca_adam_step_groups "
                         "takes at most 256")
    return dict(seg_end=seg_end, lr_scale=lr_scale, wd_scale=wd_scale, tensors=tensors)


class STEngine:
    """Forward / train-step of an ``models.ST`` through the pca_st_* entry points."""

    def __init__(self, model, B: int, N: int, mode: int = _lib.MODE_F32, training: bool = True):
        self.model = model
        self.flat = flatten_parameters(model)
        _need_cuda(self.flat)
        self.dev = self.flat.device
        self.cfg = st_config(model, B, N, mode)
        L = lib()
        n = L.pca_st_param_count(C.byref(self.cfg))
        if n != self.flat.numel():
            raise _lib.PcaHipError(f"parameter count mismatch: engine {n}, model "
                                   f"{self.flat.numel()}: {L.pca_last_error()}")
        self.split = int(L.pca_st_bucket_split(C.byref(self.cfg)))
        self.training = training
        with torch.cuda.device(self.dev):
            self.ws = torch.empty(L.pca_st_ws_bytes(C.byref(self.cfg), int(training)),
                                  dtype=torch.uint8, device=self.dev)
            self.logits = torch.empty((B * self.cfg.k, self.cfg.C), dtype=torch.float32,
                                      device=self.dev)
            if training:
                self.grads = torch.zeros_like(self.flat)
                self.loss = torch.zeros(1, dtype=torch.float32, device=self.dev)
                self.stats = torch.zeros(2, dtype=torch.float32, device=self.dev)
        # the set-resident forward's bounded spin-waits (csrc/set128_fwd.hip) count their expiries in a
        # word of the workspace that only the caller clears: zero it now, look at it at every host sync
        self._handoff_word = None
        if training:
            ptr = C.c_void_p()
            check(L.pca_st_handoff_counter(C.byref(self.cfg), self.ws.data_ptr(), C.byref(ptr)),
                  "pca_st_handoff_counter")
            if ptr.value:
                off = ptr.value - self.ws.data_ptr()
                self._handoff_word = self.ws[off:off + 4].view(torch.int32)
                self._handoff_word.zero_()

    def reproducible(self, lengths: bool = False) -> bool:
        """Whether the library guarantees that two identical ``fwd_bwd`` calls of this engine (with
        ``lengths``, if set) give identical bits: logits, loss, statistics and every gradient, launched
        eagerly or replayed from a graph (pca_st_step_reproducible)."""
        return bool(lib().pca_st_step_reproducible(C.byref(self.cfg), int(bool(lengths))))

    @property
    def bit_reproducible(self) -> bool:
        """``reproducible()`` for dense batches: True for the fused d = 128 / d = 256 steps and the d = 64
        step of the shipped shapes in the bf16 mode (B <= 256), False in the exact fp32 mode."""
        return self.reproducible(False)

    def check_handoffs(self) -> None:
        """Raise if a pair hand-off of the set-resident forward ever timed out (one host sync): a
        workgroup whose partner was not scheduled within ~1 s went on with stale data, i.e. every
        result since is garbage - e.g. another process holding compute units of this GPU."""
        if self._handoff_word is not None:
            n = int(self._handoff_word.item())
            if n:
                raise _lib.PcaHipError(
                    f"set-resident forward: {n} pair hand-off(s) timed out - the step's results are "
                    "invalid (is another process using this GPU?); PCA_SET128=0 selects the per-block "
                    "launches, which need no co-resident workgroups")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    @staticmethod
    def _len_ptr(lengths, B):
        if lengths is None:
            return None
        assert lengths.is_cuda and lengths.dtype == torch.int32 and lengths.is_contiguous()
        assert tuple(lengths.shape) == (B,), lengths.shape
        return lengths.data_ptr()

    def _params_ptr(self, params: Optional[torch.Tensor]) -> int:
        """The weights a forward reads: the model's flat vector, or ``params`` in its place."""
        if params is None:
            return self.flat.data_ptr()
        assert params.is_cuda and params.dtype == torch.float32 and params.is_contiguous()
        assert params.device == self.dev and tuple(params.shape) == tuple(self.flat.shape), params.shape
        assert params.data_ptr() % 16 == 0, "params must be 16-byte aligned, as the model's vector is"
        return params.data_ptr()

    def forward(self, X: torch.Tensor, lengths: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None,
                params: Optional[torch.Tensor] = None) -> torch.Tensor:
        """lengths (optional, device int32[B]): valid points per set of a padded batch.
        out (optional, device float32 [B * k, C], contiguous): where the logits go instead of the
        engine's own buffer (e.g. a slice of the buffer that holds a whole pass).
        params (optional, flat device float32 vector of the engine's size): the weights to use in place
        of the model's own (e.g. ``Trainer.averaged``)."""
        assert X.is_cuda and X.dtype == torch.float32 and X.is_contiguous()
        assert tuple(X.shape) == (self.cfg.B, self.cfg.N, self.cfg.din), X.shape
        if out is None:
            out = self.logits
        else:
            assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
            assert tuple(out.shape) == tuple(self.logits.shape), out.shape
        check(lib().pca_st_forward(C.byref(self.cfg), self._params_ptr(params), X.data_ptr(),
                                   self._len_ptr(lengths, self.cfg.B), out.data_ptr(),
                                   self.ws.data_ptr(), self._stream()),
              "pca_st_forward")
        return out

    def attention(self, X: torch.Tensor, lengths: Optional[torch.Tensor] = None, want_key: bool = True,
                  want_attn: bool = True, key_out: Optional[torch.Tensor] = None,
                  params: Optional[torch.Tensor] = None):
        """(logits, attn, key) of one inference call (pca_st_pool_attention): the logits ``forward``
        returns, bit for bit, the pooling attention attn [B, k, h, N] of dec.0 (modules.PMA.attention) and
        key [B, N], its mean over seeds and heads (what pca_hip.select_points sorts by).  attn / key are
        None without ``want_attn`` / ``want_key``.  The tensors are the engine's own buffers, overwritten
        by the next call; ``key_out`` (device float32 [B, N], contiguous) receives the key instead.
        fp32 whatever the engine's mode; not differentiable.  Needs an engine built with training=False.
        ``params``: as in ``forward``."""
        if self.training:
            raise _lib.PcaHipError("STEngine.attention needs an engine built with training=False")
        assert X.is_cuda and X.dtype == torch.float32 and X.is_contiguous()
        cfg = self.cfg
        assert tuple(X.shape) == (cfg.B, cfg.N, cfg.din), X.shape
        L = lib()
        with torch.cuda.device(self.dev):
            if getattr(self, "_attn", None) is None:
                n = L.pca_st_pool_attention_ws_bytes(C.byref(cfg))
                if n == 0:
                    raise _lib.PcaHipError("pca_st_pool_attention_ws_bytes: " + L.pca_last_error().decode())
                # the inference workspace with the attention scratch behind it (nothing in it outlives a call)
                self.ws = torch.empty(n, dtype=torch.uint8, device=self.dev)
                self._attn = torch.empty((cfg.B, cfg.k, cfg.h, cfg.N), dtype=torch.float32, device=self.dev)
                self._key = torch.empty((cfg.B, cfg.N), dtype=torch.float32, device=self.dev)
        attn = self._attn if want_attn else None
        key = None
        if want_key:
            key = self._key if key_out is None else key_out
            assert key.is_cuda and key.dtype == torch.float32 and key.is_contiguous()
            assert tuple(key.shape) == (cfg.B, cfg.N), key.shape
        check(L.pca_st_pool_attention(C.byref(cfg), self._params_ptr(params), X.data_ptr(),
                                      self._len_ptr(lengths, cfg.B), self.logits.data_ptr(),
                                      None if attn is None else attn.data_ptr(),
                                      None if key is None else key.data_ptr(),
                                      self.ws.data_ptr(), self._stream()), "pca_st_pool_attention")
        return self.logits, attn, key

    def fwd_bwd(self, X: torch.Tensor, labels: torch.Tensor, phase: int = -1,
                grad_scale: float = 1.0, lengths: Optional[torch.Tensor] = None,
                labels2: Optional[torch.Tensor] = None, weight: Optional[torch.Tensor] = None,
                label_smoothing: float = 0.0) -> None:
        """One training step's forward, loss and backward.  ``labels2`` int64[B] / ``weight`` float32[B]
        / ``label_smoothing``: the soft targets of pca_st_train_fwd_bwd_soft (the second class of each
        set, the weight of ``labels``, the smoothing); ``stats`` then counts accuracy against the
        dominant label.  With none of them set this is the hard-label call, as before."""
        if labels2 is not None or weight is not None or label_smoothing != 0.0:
            assert labels2 is None or (labels2.is_cuda and labels2.dtype == torch.int64
                                       and labels2.numel() == self.cfg.B)
            assert weight is None or (weight.is_cuda and weight.dtype == torch.float32
                                      and weight.numel() == self.cfg.B)
            soft = _lib.PcaSoftTargets(None if labels2 is None else labels2.data_ptr(),
                                       None if weight is None else weight.data_ptr(),
                                       float(label_smoothing))
            check(lib().pca_st_train_fwd_bwd_soft(C.byref(self.cfg), self.flat.data_ptr(), X.data_ptr(),
                                                  self._len_ptr(lengths, self.cfg.B), labels.data_ptr(),
                                                  C.byref(soft), self.grads.data_ptr(),
                                                  self.loss.data_ptr(), self.stats.data_ptr(),
                                                  self.logits.data_ptr(), grad_scale, phase,
                                                  self.ws.data_ptr(), self._stream()),
                  "pca_st_train_fwd_bwd_soft")
            return
        check(lib().pca_st_train_fwd_bwd(C.byref(self.cfg), self.flat.data_ptr(), X.data_ptr(),
                                         self._len_ptr(lengths, self.cfg.B),
                                         labels.data_ptr(), self.grads.data_ptr(),
                                         self.loss.data_ptr(), self.stats.data_ptr(),
                                         self.logits.data_ptr(), grad_scale, phase,
                                         self.ws.data_ptr(), self._stream()),
              "pca_st_train_fwd_bwd")


class Trainer:
    """Data-parallel trainer: one instance per process / GPU.

    dataset   object with ``batch(idx, out=, labels_out=)`` (dataset.ESC_pc / ESC_pc_temp)
    The step consumes ``batch_size`` sets per GPU; indices come from a per-epoch device
    permutation (rank r takes r::world, DistributedSampler semantics).
    """

    def __init__(self, model, dataset, batch_size: int, lr: float = 1e-3,
                 weight_decay: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 mode: int = _lib.MODE_F32, use_graph: bool = True, seed: int = 0,
                 shuffle: bool = True, process_group=None, keep_grads: bool = False,
                 overlap: Optional[bool] = None, max_grad_norm: Optional[float] = None,
                 skip_nonfinite: bool = False, lr_schedule=None,
                 schedule_steps: Optional[int] = None, label_smoothing: float = 0.0,
                 decoupled_weight_decay: bool = False, param_groups=None,
                 average_decay: Optional[float] = None, average_start: int = 1,
                 eval_weights: str = "model"):
        """label_smoothing: eps in [0, 1) of the loss's targets.  A dataset with ``soft_targets``
        (dataset.ESC_wave_pc(..., mix_targets=True)) makes the step train on mixed labels: the frame
        launch writes the second label and the label weight of every slot into buffers the Trainer
        owns, and the loss stage reads them - no launch more, and no new state to save (the targets come
        from the draws that resume exactly).  ``read_stats`` then counts accuracy against the dominant
        label.  With 0 and a dataset without ``soft_targets`` the step is enqueued as it always was.
        max_grad_norm: clip the (rank-averaged) gradient to this global L2 norm before Adam
        (torch.nn.utils.clip_grad_norm_).  skip_nonfinite: a step whose gradient norm is inf / NaN
        changes neither parameters nor moments.  lr_schedule: the learning rate per step (step 1
        first; the last entry holds from there on) as a sequence of floats, or a callable
        step -> lr with ``schedule_steps``; it lives in a device table, so a captured step follows it
        without a re-capture.  All three at their defaults: the plain pca_adam_step launch.
        decoupled_weight_decay: torch.optim.AdamW's decay, on the weights themselves, instead of the
        coupled L2 of torch.optim.Adam.  param_groups: a sequence of (regex, lr_scale, wd_scale) matched
        with ``re.search`` against each tensor's state_dict key, first match wins (``no_decay_groups()``
        is the usual preset; ``lr_scale`` 0 freezes a tensor).  average_decay (in [0, 1)): keep an
        exponential moving average of the weights in ``averaged``, a flat device vector updated inside
        the step from applied step ``average_start`` on (a copy of the weights up to it); the same on
        every rank.  Any of the four makes the optimiser launch pca_adam_step_groups, still one launch;
        none of them: the step is enqueued as before.
        eval_weights: which weights the held-out pass of ``fit`` scores, "model" (default), "averaged"
        (needs ``average_decay``) or "both"; also an attribute, read when ``fit`` is called."""
        self.ds = dataset
        self.label_smoothing = float(label_smoothing)
        if not 0.0 <= self.label_smoothing < 1.0:
            raise ValueError(f"label_smoothing must be in [0, 1), got {label_smoothing}")
        self.keep_grads = keep_grads    # True: gradients of the last step stay readable
        self.B = int(batch_size)
        self.N = int(dataset.num_points)
        self.eng = STEngine(model, self.B, self.N, mode, training=True)
        self.dev = self.eng.dev
        self.lr, self.wd, self.betas, self.eps = lr, weight_decay, betas, eps
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(process_group) if dist.is_initialized() else 0
        self.seed = seed
        self.shuffle = shuffle
        self.use_graph = use_graph
        n = self.eng.flat.numel()
        with torch.cuda.device(self.dev):
            self.m = torch.zeros(n, dtype=torch.float32, device=self.dev)
            self.v = torch.zeros(n, dtype=torch.float32, device=self.dev)
            self.step_count = torch.zeros(2, dtype=torch.int32, device=self.dev)  # [count, ticket]
            self.idx = torch.zeros(self.B, dtype=torch.int64, device=self.dev)
            self.X = torch.empty((self.B, self.N, self.eng.cfg.din), dtype=torch.float32,
                                 device=self.dev)
            self.labels = torch.zeros(self.B, dtype=torch.int64, device=self.dev)
            # soft targets (dataset.soft_targets): second label and weight of the first, per slot
            self.labels2 = self.weight = None
            if getattr(dataset, "soft_targets", False):
                self.labels2 = torch.zeros(self.B, dtype=torch.int64, device=self.dev)
                self.weight = torch.ones(self.B, dtype=torch.float32, device=self.dev)
            # padded batches of variable-size sets (dataset.variable_length): point counts
            self.lengths = (torch.zeros(self.B, dtype=torch.int32, device=self.dev)
                            if getattr(dataset, "variable_length", False) else None)
            # device cursor: the epoch's index batches live in ``seq``; the pack kernel takes
            # batch (step_count - epoch_base), so a step is a bare graph replay
            self.epoch_base = torch.zeros(1, dtype=torch.int32, device=self.dev)
            self.seq = None
            # Several GPUs, two ways to exchange the gradients:
            #   overlap=True : the step is split at the bucket boundary; bucket A (enc.1 + dec) is
            #                  reduced on a side stream under enc.0's backward, bucket B after it
            #   overlap=False: one all-reduce of the whole vector between backward and Adam
            # The split costs three graph launches instead of one and ends the launch merging of
            # the backward at the boundary: measured +82 us per step at cfg2 on one GPU
            # (PCA_FORCE_SPLIT=1: 0.370 -> 0.452 ms), more than the all-reduce of 1.2 MB it can
            # hide.  Default: overlap only from 16 MB of gradients on.
            if overlap is None:
                overlap = self.eng.flat.numel() * 4 >= (16 << 20)
            self._split = (self.world > 1 and bool(overlap)) or \
                os.environ.get("PCA_FORCE_SPLIT") == "1"
            # (PCA_FORCE_SPLIT=2: the overlap=False step shape on one GPU, minus the all-reduce)
            self._exchange = self.world > 1 or os.environ.get("PCA_FORCE_SPLIT") == "2"
            # third form (set_exchange("captured")): the all-reduce is captured INSIDE the step's one
            # graph, [pack .. backward | all-reduce | Adam] = one graph launch per step
            self._captured = False
            self.comm_stream = torch.cuda.Stream(self.dev) if self._split else None
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        if self.max_grad_norm is not None and not self.max_grad_norm > 0.0:
            raise ValueError(f"max_grad_norm must be positive, got {max_grad_norm}")
        self.skip_nonfinite = bool(skip_nonfinite)
        table = _lr_table(lr_schedule, schedule_steps)
        self._optim_on = (self.max_grad_norm is not None or self.skip_nonfinite
                          or table is not None)
        self.lr_table = self.optim_state = self.norm_partials = None
        if self._optim_on:
            with torch.cuda.device(self.dev):
                self.lr_table = None if table is None else table.to(self.dev)
                if self.max_grad_norm is not None or self.skip_nonfinite:
                    self.norm_partials = torch.zeros(int(lib().pca_grad_sumsq_partials(n)),
                                                     dtype=torch.float64, device=self.dev)
        # AdamW, per-tensor groups, the averaged copy: any of them selects pca_adam_step_groups
        self.decoupled = bool(decoupled_weight_decay)
        self.average_decay = None if average_decay is None else float(average_decay)
        self.average_start = int(average_start)
        if self.average_decay is not None and not 0.0 <= self.average_decay < 1.0:
            raise ValueError(f"average_decay must be in [0, 1), got {average_decay}")
        if self.average_start < 1:
            raise ValueError(f"average_start must be >= 1, got {average_start}")
        self.groups = None if param_groups is None else resolve_param_groups(model, param_groups)
        self._groups_on = (self.decoupled or self.groups is not None
                           or self.average_decay is not None)
        self.averaged = self._seg_end = self._seg_lr = self._seg_wd = self._seg_end_host = None
        if self._optim_on or self._groups_on:
            with torch.cuda.device(self.dev):
                # pca_optim_state, 32 bytes: [skipped, clipped, last_norm, last_lr, norm_sum(2), count, -]
                self.optim_state = torch.zeros(8, dtype=torch.int32, device=self.dev)
                if self.groups is not None:
                    ends = self.groups["seg_end"]
                    assert ends[-1] == n, (ends[-1], n)
                    self._seg_end_host = (C.c_int64 * len(ends))(*ends)
                    self._seg_end = torch.tensor(ends, dtype=torch.int64).to(self.dev)
                    self._seg_lr = torch.tensor(self.groups["lr_scale"], dtype=torch.float64) \
                        .to(torch.float32).to(self.dev)
                    self._seg_wd = torch.tensor(self.groups["wd_scale"], dtype=torch.float64) \
                        .to(torch.float32).to(self.dev)
                if self.average_decay is not None:
                    # up to ``average_start`` the step overwrites it with the weights: no stale start
                    self.averaged = self.eng.flat.clone()
        self._cursor_mode = callable(getattr(dataset, "batch_seq", None))
        self._k = 0                       # optimiser steps issued so far (host copy)
        self.g0 = self.g1 = self.g2 = None
        self._draw_frozen = None          # see _capture
        self._evaluator = None            # fit's held-out pass, built once
        self._evaluator_avg = None        # the same pass on ``averaged``
        self.eval_weights = eval_weights
        self._check_eval_weights()
        self.indices = ShardedIndexStream(len(dataset), self.B, self.rank, self.world, seed,
                                          shuffle, self.dev)
        if self.world > 1:      # identical initial weights on every rank (rank 0's)
            dist.broadcast(self.eng.flat, src=0, group=self.pg)
            if self.averaged is not None:
                self.averaged.copy_(self.eng.flat)

    @property
    def bit_reproducible(self) -> bool:
        """Whether the library guarantees this Trainer's forward + backward bit for bit (STEngine.reproducible,
        for the batches of this dataset: padded ones if it is ``variable_length``): then a graph replay equals
        the eager launches, and a run resumed from ``state_dict()`` equals the uninterrupted one."""
        return self.eng.reproducible(self.lengths is not None)

    # ---- how the gradients are exchanged ---------------------------------------------
    def set_exchange(self, form: str) -> None:
        """Choose the step shape of a multi-rank run and drop the captured graphs (the next step
        re-captures).  "serial": [graph: pack .. backward] -> all-reduce of the whole vector -> Adam;
        "overlap": the step split at the bucket boundary, bucket A reduced on a side stream under
        enc.0's backward; "captured": ONE graph per step with the all-reduce recorded inside it
        (needs a backend whose collectives can be stream-captured: RCCL / nccl);
        "captured_overlap": ONE graph per step as well, split at the bucket boundary INSIDE it - bucket A's
        all-reduce forks onto a side stream under enc.0's backward and joins before Adam (the overlap of
        "overlap" without its three graph launches and cross-stream events per step, which cost 68 us).
        bench.py times all of them on the first windows of a multi-GPU run and keeps the fastest."""
        if form not in ("serial", "overlap", "captured", "captured_overlap"):
            raise ValueError(form)
        torch.cuda.synchronize(self.dev)
        self.g0 = self.g1 = self.g2 = None
        multi = self.world > 1 or (dist.is_initialized() and os.environ.get("PCA_EXCHANGE_WORLD1") == "1")
        self._split = form in ("overlap", "captured_overlap") and multi
        self._captured = form in ("captured", "captured_overlap") and multi
        self._exchange = multi
        if self._split and self.comm_stream is None:
            self.comm_stream = torch.cuda.Stream(self.dev)
        self.exchange_form = form

    def _allreduce_all(self):
        if self.world > 1 or self._captured:
            dist.all_reduce(self.eng.grads, group=self.pg)

    def _captured_body(self):
        """[pack .. backward | all-reduce | Adam] as it is recorded into (or, without graphs, run as) one
        step.  Split form: bucket A (enc.1 + dec, final after phase 0) is reduced on the side stream
        while enc.0's backward runs on the main one; both join before Adam."""
        self._seg0()
        if not self._split:
            self._seg1()
            self._allreduce_all()
        else:
            main = torch.cuda.current_stream(self.dev)
            self.comm_stream.wait_stream(main)                    # fork
            second = allreduce_buckets(self.eng.grads, self.eng.split, self.pg, self.comm_stream)
            self._seg1()
            second()                                              # bucket B on the main stream
            main.wait_stream(self.comm_stream)                    # join
        self._seg2()

    # ---- index stream ------------------------------------------------------------
    def _next_indices(self) -> torch.Tensor:
        return self.indices.next()

    # ---- the three device segments of a step ---------------------------------------
    def _soft_kw(self) -> dict:
        """What ``fwd_bwd`` takes beyond the hard step; empty: the hard step, as enqueued before."""
        kw = {}
        if self.labels2 is not None:
            kw.update(labels2=self.labels2, weight=self.weight)
        if self.label_smoothing != 0.0:
            kw.update(label_smoothing=self.label_smoothing)
        return kw

    def _seg0(self):     # pack + zero grads + forward + loss + backward(dec, enc.1)
        tk = {} if self.labels2 is None else dict(labels2_out=self.labels2, weight_out=self.weight)
        if self._cursor_mode:
            kw = dict(lengths_out=self.lengths) if self.lengths is not None else {}
            # the pack rides in the engine's first launch (pca_pack_defer): one launch less per step
            defer = os.environ.get("PCA_PACK_DEFER", "1") != "0"
            if defer:
                check(lib().pca_pack_defer(1), "pca_pack_defer")
            try:
                self.ds.batch_seq(self.seq, self.step_count, self.epoch_base, self.B, out=self.X,
                                  labels_out=self.labels, **kw)
                if self.keep_grads:
                    self.eng.grads.zero_()
                self.eng.fwd_bwd(self.X, self.labels, phase=0 if self._split else -1,
                                 lengths=self.lengths, **self._soft_kw())
            except BaseException:
                if defer:            # disarm (drops a pending job) without masking the error in flight
                    lib().pca_pack_defer(0)
                raise
            if defer:
                check(lib().pca_pack_defer(0), "pca_pack_defer")
            return
        elif self.lengths is not None and getattr(self.ds, "stochastic", False):
            # sets that lose random points (the waveform datasets' masks in drop mode): the point counts
            # and the fresh draw per replay both come from the one frame launch
            self.ds.batch(self.idx, out=self.X, labels_out=self.labels, lengths_out=self.lengths,
                          draw_dev=self.step_count, **tk)
        elif self.lengths is not None:
            self.ds.batch(self.idx, out=self.X, labels_out=self.labels,
                          lengths_out=self.lengths)
        elif getattr(self.ds, "stochastic", False):
            # random sub-sampling datasets: the draw number must advance per REPLAY of a captured
            # step, so it is read on the device from the optimiser's step counter
            self.ds.batch(self.idx, out=self.X, labels_out=self.labels,
                          draw_dev=self.step_count, **tk)
        else:
            self.ds.batch(self.idx, out=self.X, labels_out=self.labels, **tk)
        if self.keep_grads:           # otherwise the Adam pass leaves them cleared
            self.eng.grads.zero_()
        # one GPU: the whole backward in one call (the shared-query gradient kernels of all three
        # blocks then share one pair of launches); several GPUs: stop at the bucket boundary
        self.eng.fwd_bwd(self.X, self.labels, phase=0 if self._split else -1,
                         lengths=self.lengths, **self._soft_kw())

    def _seg1(self):     # backward(enc.0)
        if self._split:
            self.eng.fwd_bwd(self.X, self.labels, phase=1, lengths=self.lengths, **self._soft_kw())

    def _seg2(self):     # Adam over the flat vector
        e = self.eng
        L, n, st = lib(), e.flat.numel(), e._stream()
        ptr = lambda t: None if t is None else t.data_ptr()
        head = (e.flat.data_ptr(), e.grads.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), n)
        if not (self._optim_on or self._groups_on):
            check(L.pca_adam_step(*head, self.lr, self.betas[0], self.betas[1], self.eps, self.wd,
                                  1.0 / self.world, self.step_count.data_ptr(),
                                  int(not self.keep_grads), st), "pca_adam_step")
            return
        # [sum of squares ->] the guarded step: both launches where the plain one sits, i.e. after the
        # all-reduce / the join, so every rank clips the same averaged gradient and skips alike
        part, npart = None, 0
        if self.norm_partials is not None:
            part, npart = self.norm_partials.data_ptr(), self.norm_partials.numel()
            check(L.pca_grad_sumsq(e.grads.data_ptr(), n, part, npart, st), "pca_grad_sumsq")
        o = _lib.OptimCfg(self.lr, self.betas[0], self.betas[1], self.eps, self.wd,
                          1.0 / self.world, self.max_grad_norm or 0.0, int(self.skip_nonfinite))
        tab = self.lr_table
        guarded = (*head, C.byref(o), part, npart, ptr(tab), 0 if tab is None else tab.numel(),
                   self.step_count.data_ptr(), self.optim_state.data_ptr(), int(not self.keep_grads))
        if not self._groups_on:
            check(L.pca_adam_step_ex(*guarded, st), "pca_adam_step_ex")
            return
        # AdamW, the segment table and the averaged copy, in the one launch at the same place
        gr = _lib.OptimGroups(
            int(self.decoupled), 0 if self.groups is None else len(self.groups["seg_end"]),
            ptr(self._seg_end), ptr(self._seg_lr), ptr(self._seg_wd), ptr(self.averaged),
            1.0 if self.average_decay is None else 1.0 - self.average_decay, self.average_start)
        check(L.pca_adam_step_groups(*guarded, C.byref(gr), self._seg_end_host, st),
              "pca_adam_step_groups")

    def _capture(self):
        """Warm up eagerly on a side stream, then capture the segments."""
        s = torch.cuda.Stream(self.dev)
        s.wait_stream(torch.cuda.current_stream(self.dev))
        live = (self.eng.flat, self.m, self.v, self.step_count, self.eng.stats)
        if self.optim_state is not None:
            live += (self.optim_state,)
        if self.averaged is not None:
            live += (self.averaged,)
        snap = tuple(t.clone() for t in live)
        with torch.cuda.stream(s):
            self._seg0(); self._seg1(); self._seg2()
        torch.cuda.current_stream(self.dev).wait_stream(s)
        torch.cuda.synchronize(self.dev)
        for dst, src in zip(live, snap):
            dst.copy_(src)
        # thread-local capture mode: a HIP call from another thread (e.g. the RCCL watchdog of
        # torch.distributed) must not invalidate the capture
        mode = dict(capture_error_mode="thread_local")
        if self._captured:              # [pack .. backward | all-reduce | Adam] in ONE graph
            self.g0 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.g0, **mode):
                self._captured_body()
        elif not self._split and not self._exchange:
            self.g0 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.g0, **mode):
                self._seg0(); self._seg1(); self._seg2()
        elif not self._split:           # [pack, forward, backward] | all-reduce | Adam
            # (Adam is one kernel: a plain launch, not a one-node graph - every graph boundary
            #  costs tens of microseconds of GPU idle time)
            self.g0 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.g0, **mode):
                self._seg0()
        else:
            self.g0, self.g1, self.g2 = (torch.cuda.CUDAGraph() for _ in range(3))
            with torch.cuda.graph(self.g0, **mode):
                self._seg0()
            with torch.cuda.graph(self.g1, pool=self.g0.pool(), **mode):
                self._seg1()
            with torch.cuda.graph(self.g2, pool=self.g0.pool(), **mode):
                self._seg2()
        # a stochastic dataset's host draw number is a by-value argument: the capture froze this one
        self._draw_frozen = getattr(self.ds, "_draw", None)
        for dst, src in zip(live, snap):
            dst.copy_(src)

    def step(self) -> None:
        """One optimiser step; enqueues only (no host sync)."""
        if self._cursor_mode:
            spe = self.indices.steps_per_epoch()
            if self._k % spe == 0:        # once per epoch: stage its index batches
                ep = self.indices.next_epoch()
                if self.seq is None:
                    self.seq = torch.empty(spe * self.B, dtype=torch.int64, device=self.dev)
                self.seq.copy_(ep, non_blocking=True)
                self.epoch_base.fill_(self._k)
            self._k += 1
        else:
            self.idx.copy_(self._next_indices(), non_blocking=True)
            self._k += 1
        if self.use_graph and self.g0 is None:
            self._capture()
        main = torch.cuda.current_stream(self.dev)
        if self._captured:
            if self.use_graph:
                self.g0.replay()
            else:
                self._captured_body()
            return
        if not self._split and not self._exchange:
            if self.use_graph:
                self.g0.replay()
            else:
                self._seg0(); self._seg1(); self._seg2()
            return
        e = self.eng
        if not self._split:
            self.g0.replay() if self.use_graph else self._seg0()
            if self.world > 1:
                dist.all_reduce(e.grads, group=self.pg)
            self._seg2()
            return
        self.g0.replay() if self.use_graph else self._seg0()
        # bucket A (enc.1 + dec) is final: reduce it while enc.0's backward runs
        self.comm_stream.wait_stream(main)
        if self.world > 1:
            second = allreduce_buckets(e.grads, e.split, self.pg, self.comm_stream)
        self.g1.replay() if self.use_graph else self._seg1()
        if self.world > 1:
            second()
        main.wait_stream(self.comm_stream)
        self.g2.replay() if self.use_graph else self._seg2()

    # ---- epoch statistics ------------------------------------------------------------
    def read_stats(self, reset: bool = True) -> Tuple[float, float]:
        """(sum of per-sample losses, number of correct predictions) since the last reset,
        summed over ranks.  One host sync.  On soft targets the loss is the cross-entropy against the
        mixed (and smoothed) target and a prediction counts as correct when it is the dominant label:
        the slot's own label when its weight is >= 0.5, the second label otherwise."""
        st = self.eng.stats.clone()
        if self.world > 1:
            dist.all_reduce(st, group=self.pg)
        out = st.cpu().tolist()
        self.eng.check_handoffs()
        if reset:
            self.eng.stats.zero_()
        return float(out[0]), float(out[1])

    def _optim_fields(self) -> dict:
        """pca_optim_state as plain values (one host read)."""
        host = self.optim_state.cpu()
        f32, f64 = host.view(torch.float32), host.view(torch.float64)
        return dict(skipped=int(host[0]), clipped=int(host[1]), last_norm=float(f32[2]),
                    last_lr=float(f32[3]), norm_sum=float(f64[2]), norm_count=int(host[6]))

    def read_optim_stats(self, reset: bool = True) -> dict:
        """grad_norm_mean (over the finite steps since the last reset), last_grad_norm, lr (of the last
        step), clipped and skipped (steps, since the start of the run).  The norm is that of the
        gradient Adam used, before clipping; 0 when neither clipping nor skipping is on.  One host
        read; ``reset`` clears the mean's accumulator."""
        if self.optim_state is None:
            raise _lib.PcaHipError("read_optim_stats: this Trainer was built without max_grad_norm, "
                                   "skip_nonfinite, lr_schedule, decoupled_weight_decay, param_groups "
                                   "or average_decay")
        f = self._optim_fields()
        if reset:
            self.optim_state[4:7].zero_()
        return dict(grad_norm_mean=f["norm_sum"] / f["norm_count"] if f["norm_count"] else 0.0,
                    last_grad_norm=f["last_norm"], lr=f["last_lr"], clipped=f["clipped"],
                    skipped=f["skipped"])

    def _check_eval_weights(self) -> str:
        if self.eval_weights not in ("model", "averaged", "both"):
            raise ValueError(f"eval_weights must be 'model', 'averaged' or 'both', got "
                             f"{self.eval_weights!r}")
        if self.eval_weights != "model" and self.average_decay is None:
            raise ValueError(f"eval_weights={self.eval_weights!r} needs a Trainer built with "
                             "average_decay")
        return self.eval_weights

    def averaged_state_dict(self) -> dict:
        """``averaged`` under the model's state_dict keys, as CPU tensors of the parameters' shapes (one
        host sync): what ``load_state_dict`` of a second model, or ``runfiles.save_run(state_dict=)``,
        takes to use or write the averaged weights in the reference's layout."""
        if self.averaged is None:
            raise _lib.PcaHipError("averaged_state_dict: this Trainer was built without average_decay")
        model = getattr(self.eng.model, "module", self.eng.model)
        host = self.averaged.detach().to("cpu")
        out, off = {}, 0
        for key, p in model.state_dict().items():
            out[key] = host[off:off + p.numel()].view(p.shape).clone()
            off += p.numel()
        assert off == host.numel()
        return out

    # ---- exact resume ----------------------------------------------------------------
    def state_dict(self) -> dict:
        """Everything the next step depends on, as CPU tensors and plain values (one host sync): legal
        at any step boundary, mid-epoch included.  The staged epoch sequence and the current
        permutation are not stored: ``load_state_dict`` re-derives them from (seed, epoch)."""
        cpu = lambda t: t.detach().to("cpu").clone()
        optim = {}
        if self.optim_state is not None:
            # the state words as they are (norm_sum keeps its fp64 bits) next to the readable fields
            optim = dict(optim=dict(self._optim_fields(), words=cpu(self.optim_state),
                                    lr_schedule=None if self.lr_table is None else cpu(self.lr_table),
                                    max_grad_norm=self.max_grad_norm,
                                    skip_nonfinite=self.skip_nonfinite))
        if self._groups_on:
            optim["optim"].update(self._groups_options())
            if self.averaged is not None:
                optim["avg"] = cpu(self.averaged)
        return dict(format=1, B=self.B, N=self.N, mode=int(self.eng.cfg.mode), world=int(self.world),
                    flat=cpu(self.eng.flat), m=cpu(self.m), v=cpu(self.v),
                    step_count=int(self.step_count[0].item()), k=int(self._k),
                    epoch_base=int(self.epoch_base.item()), stats=cpu(self.eng.stats),
                    stream=self.indices.state(),
                    # stochastic datasets: the host half of the draw number (the device half is
                    # step_count); a captured step froze draw_frozen
                    draw=getattr(self.ds, "_draw", None), draw_frozen=self._draw_frozen, **optim)

    def load_state_dict(self, state: dict) -> None:
        """Continue a run bit for bit from ``state_dict()``.  B, N, mode and world must be this
        trainer's (a mismatch raises and names the field).  Captured graphs are dropped: the next
        step re-captures."""
        mine = dict(B=self.B, N=self.N, mode=int(self.eng.cfg.mode), world=int(self.world))
        for name, have in mine.items():
            if int(state[name]) != have:
                raise ValueError(f"checkpoint mismatch: {name} is {state[name]} in the checkpoint, "
                                 f"{have} in this trainer")
        if state["flat"].numel() != self.eng.flat.numel():
            raise ValueError(f"checkpoint mismatch: parameters is {state['flat'].numel()} in the "
                             f"checkpoint, {self.eng.flat.numel()} in this trainer")
        self._check_optim(state.get("optim"))
        torch.cuda.synchronize(self.dev)
        self.g0 = self.g1 = self.g2 = None
        if self.optim_state is not None:
            self.optim_state.copy_(state["optim"]["words"])
        if self.averaged is not None:
            self.averaged.copy_(state["avg"])
        # into the vectors the engines (and the module's parameters) are views of, never a re-bind
        self.eng.flat.copy_(state["flat"])
        self.m.copy_(state["m"])
        self.v.copy_(state["v"])
        self.eng.stats.copy_(state["stats"])
        self.step_count.zero_()
        self.step_count[0] = int(state["step_count"])
        self.epoch_base.fill_(int(state["epoch_base"]))
        self._k = int(state["k"])
        self.indices.load_state(state["stream"])
        if self._cursor_mode and self.indices.epoch > 0:
            # the epoch in progress: its index batches as next_epoch() staged them
            spe = self.indices.steps_per_epoch()
            if self.seq is None:
                self.seq = torch.empty(spe * self.B, dtype=torch.int64, device=self.dev)
            self.seq.copy_(self.indices._perm[:spe * self.B])
        if state.get("draw") is not None and hasattr(self.ds, "_draw"):
            frozen = state.get("draw_frozen")
            # the re-capture (one eager warm-up, one recorded call) must freeze the same number
            self.ds._draw = int(frozen) - 2 if (self.use_graph and frozen is not None) \
                else int(state["draw"])
        self._draw_frozen = None

    def _groups_options(self) -> dict:
        """The options of pca_adam_step_groups as a checkpoint stores them: plain values and CPU tensors
        (the segment table with its scales as the launch reads them, None without param_groups)."""
        cpu = lambda t: None if t is None else t.detach().to("cpu").clone()
        return dict(decoupled=self.decoupled, seg_end=cpu(self._seg_end), seg_lr_scale=cpu(self._seg_lr),
                    seg_wd_scale=cpu(self._seg_wd), average_decay=self.average_decay,
                    average_start=self.average_start if self.average_decay is not None else None)

    def _check_optim(self, saved: Optional[dict]) -> None:
        """The checkpoint's optimiser options against this trainer's; a difference raises, naming it.
        A checkpoint from before the AdamW / groups / averaging options holds none of them: it is one
        with all of them off."""
        mine = dict(max_grad_norm=self.max_grad_norm, skip_nonfinite=self.skip_nonfinite)
        theirs = dict(max_grad_norm=None, skip_nonfinite=False) if saved is None else saved
        for name, have in mine.items():
            if theirs[name] != have:
                raise ValueError(f"checkpoint mismatch: {name} is {theirs[name]} in the checkpoint, "
                                 f"{have} in this trainer")
        off = dict(decoupled=False, seg_end=None, seg_lr_scale=None, seg_wd_scale=None,
                   average_decay=None, average_start=None)
        got = {k: (saved or {}).get(k, v) for k, v in off.items()}
        want = self._groups_options()
        for key, name in (("decoupled", "decoupled_weight_decay"), ("average_decay", "average_decay"),
                          ("average_start", "average_start")):
            if got[key] != want[key]:
                raise ValueError(f"checkpoint mismatch: {name} is {got[key]} in the checkpoint, "
                                 f"{want[key]} in this trainer")
        for key in ("seg_end", "seg_lr_scale", "seg_wd_scale"):
            a, b = got[key], want[key]
            if (a is None) != (b is None) or (a is not None and not (a.shape == b.shape
                                                                     and torch.equal(a, b))):
                describe = lambda t: "absent" if t is None else f"{t.numel()} segments {t.tolist()}"
                raise ValueError(f"checkpoint mismatch: param_groups ({key}) is {describe(a)} in the "
                                 f"checkpoint, {describe(b)} in this trainer")
        tab = None if saved is None else saved.get("lr_schedule")
        mine_tab = None if self.lr_table is None else self.lr_table.cpu()
        if (tab is None) != (mine_tab is None) or (
                tab is not None and not (tab.shape == mine_tab.shape and torch.equal(tab, mine_tab))):
            describe = lambda t: "absent" if t is None else f"a table of {t.numel()} steps"
            raise ValueError(f"checkpoint mismatch: lr_schedule is {describe(tab)} in the checkpoint, "
                             f"{describe(mine_tab)} in this trainer"
                             + ("" if tab is None or mine_tab is None or tab.shape != mine_tab.shape
                                else " with other values"))

    # ---- the reference's epoch loop --------------------------------------------------------
    def fit(self, epochs: int, test_dataset=None, eval_every: int = 10,
            checkpoint_path: Optional[str] = None, checkpoint_every: Optional[int] = None,
            log=print) -> list:
        """Code/settransformer.py:96-131: ``steps_per_epoch`` steps per epoch, the train loss and
        accuracy of the epoch (one ``read_stats``), the held-out pass over ``test_dataset`` at
        ``epoch % eval_every == 0`` (one ``Evaluator.run``), the reference's two lines through ``log``.
        Starts at the epoch this trainer is in (0, or where a loaded state stopped; an epoch in
        progress is finished first) and runs up to epoch ``epochs - 1``.  With ``checkpoint_path`` a
        checkpoint (runfiles.save_checkpoint) is written every ``checkpoint_every`` epochs (default:
        every epoch) and after the last.  The only host syncs are those reads (and a checkpoint's).
        Returns one dict per epoch run: epoch, train_loss, train_acc and, where the held-out pass
        ran, test_loss, test_acc, test_topk_acc.  A trainer with max_grad_norm, skip_nonfinite or
        lr_schedule adds grad_norm (mean over the epoch's finite steps), lr (of the epoch's last
        step), clipped_steps and skipped_steps (since the start of the run): one more host read
        (``read_optim_stats``) and one more line per epoch.
        ``self.eval_weights`` (``Trainer(eval_weights=)``, or set before the call) says which weights
        the held-out pass scores.  "model" (default): the model's.
        "averaged" (needs ``average_decay``): ``averaged``, reported under the same test_* names.
        "both": the model's as before, and test_avg_loss, test_avg_acc, test_avg_topk_acc from a second
        ``Evaluator.run`` on ``averaged`` (one more host read per evaluated epoch, one more line)."""
        eval_weights = self._check_eval_weights()
        spe = self.indices.steps_per_epoch()
        if test_dataset is not None and eval_weights != "averaged" and (
                self._evaluator is None or self._evaluator.ds is not test_dataset):
            self._evaluator = Evaluator(self.eng.model, test_dataset, self.B,
                                        int(self.eng.cfg.mode), process_group=self.pg)
        if test_dataset is not None and eval_weights != "model" and (
                self._evaluator_avg is None or self._evaluator_avg.ds is not test_dataset):
            self._evaluator_avg = Evaluator(self.eng.model, test_dataset, self.B,
                                            int(self.eng.cfg.mode), process_group=self.pg
                                            ).use_params(self.averaged)
        history = []
        first = self._k // spe
        for epoch in range(first, int(epochs)):
            for _ in range(spe - (self._k - epoch * spe)):
                self.step()
            loss_sum, correct = self.read_stats()
            seen = spe * self.B * self.world
            entry = dict(epoch=epoch, train_loss=loss_sum / seen, train_acc=correct / seen)
            log(f"Epoch {epoch}: train loss {entry['train_loss']:.3f} train acc "
                f"{entry['train_acc']:.3f}")
            if self._optim_on:
                o = self.read_optim_stats()
                entry.update(grad_norm=o["grad_norm_mean"], lr=o["lr"], clipped_steps=o["clipped"],
                             skipped_steps=o["skipped"])
                log(f"Epoch {epoch}: grad norm {o['grad_norm_mean']:.3f} lr {o['lr']:.3e} clipped "
                    f"{o['clipped']} skipped {o['skipped']}")
            if test_dataset is not None and epoch % eval_every == 0:
                res = (self._evaluator_avg if eval_weights == "averaged" else self._evaluator).run()
                entry.update(test_loss=res["loss"], test_acc=res["acc"],
                             test_topk_acc=res["topk_acc"])
                log(f"Epoch {epoch}: test loss {res['loss']:.3f} test acc {res['acc']:.3f}")
                if eval_weights == "both":
                    res = self._evaluator_avg.run()
                    entry.update(test_avg_loss=res["loss"], test_avg_acc=res["acc"],
                                 test_avg_topk_acc=res["topk_acc"])
                    log(f"Epoch {epoch}: averaged weights test loss {res['loss']:.3f} test acc "
                        f"{res['acc']:.3f}")
            history.append(entry)
            if checkpoint_path is not None and self.rank == 0 and (
                    (epoch + 1) % (checkpoint_every or 1) == 0 or epoch + 1 == int(epochs)):
                import runfiles
                runfiles.save_checkpoint(checkpoint_path, self)
        return history


@torch.no_grad()
def evaluate(model, dataset, batch_size: int, mode: int = _lib.MODE_F32
             ) -> Tuple[float, int]:
    """Accuracy over ``dataset`` in order (full batches through the engine, the tail through
    a second engine sized for it).  Returns (accuracy, n)."""
    n = len(dataset)
    dev = next(model.parameters()).device
    correct = torch.zeros((), dtype=torch.int64, device=dev)
    done = 0
    while done < n:
        b = min(batch_size, n - done)
        eng = STEngine(model, b, dataset.num_points, mode, training=False)
        while done + b <= n:
            idx = torch.arange(done, done + b, device=dev)
            res = dataset.batch(idx)
            X, lab = res[0], res[1]
            logits = eng.forward(X, res[2] if len(res) > 2 else None)
            correct += (logits.argmax(1) == lab).sum()
            done += b
    return float(correct) / max(n, 1), n


class Evaluator:
    """The held-out pass of Code/settransformer.py:117-131 as a persistent object.

    Built once: one ``STEngine`` for full batches and one for the tail of this rank's shard, on the
    flat parameter vector the model already has (``flatten_parameters`` is idempotent, so after a
    ``Trainer`` was built on ``model`` these engines read the very vector its Adam step updates: no
    copy, and a ``run()`` after a ``step()`` sees the new weights).  Rank r of ``process_group``
    scores the contiguous shard [r * n // world, (r + 1) * n // world) in order; nothing is dropped.

    ``run()``: every batch's logits go into one device buffer, one ``pca_eval_metrics`` call scores
    it, the int64 counters and confusion matrix are all-reduced in one message and the fp64 loss in
    another, and the host reads once.  Nothing waits on the device per batch.
    """

    def __init__(self, model, dataset, batch_size: int, mode: int = _lib.MODE_F32, topk: int = 5,
                 process_group=None):
        self.ds, self.topk, self.pg = dataset, int(topk), process_group
        self.params = None                # see use_params
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(process_group) if dist.is_initialized() else 0
        self.n = len(dataset)
        lo, hi = self.rank * self.n // self.world, (self.rank + 1) * self.n // self.world
        self.n_local = hi - lo
        self.B = max(1, min(int(batch_size), self.n_local))
        N = int(dataset.num_points)
        varlen = bool(getattr(dataset, "variable_length", False))
        flat = flatten_parameters(model)
        _need_cuda(flat)
        self.dev = flat.device
        self.engines = []                 # (engine, X, lengths), full batches first
        for b in (self.B if self.n_local else 0, self.n_local % self.B):
            if b:
                eng = STEngine(model, b, N, mode, training=False)
                assert eng.flat.data_ptr() == flat.data_ptr()
                if eng.cfg.k != 1:
                    raise _lib.PcaHipError(f"Evaluator scores one logit row per set; the model has "
                                           f"{eng.cfg.k} outputs per set")
                with torch.cuda.device(self.dev):
                    X = torch.empty((b, N, eng.cfg.din), dtype=torch.float32, device=self.dev)
                    ln = torch.zeros(b, dtype=torch.int32, device=self.dev) if varlen else None
                self.engines.append((eng, X, ln))
        self.C = int(st_config(model, 1, N, mode).C)
        with torch.cuda.device(self.dev):
            self.idx = torch.arange(lo, hi, dtype=torch.int64, device=self.dev)
            self.logits = torch.empty((self.n_local, self.C), dtype=torch.float32, device=self.dev)
            self.labels = torch.zeros(self.n_local, dtype=torch.int64, device=self.dev)
            # [4 counters | C x C confusion | the fp64 loss sum's bits]: one buffer, one host read
            self.acc = torch.zeros(4 + self.C * self.C + 1, dtype=torch.int64, device=self.dev)
        self.counts = self.acc[:4]
        self.confusion = self.acc[4:4 + self.C * self.C].view(self.C, self.C)
        self.loss_sum = self.acc[4 + self.C * self.C:].view(torch.float64)

    def use_params(self, params: Optional[torch.Tensor]) -> "Evaluator":
        """Score ``params`` (a flat device float32 vector of the model's size, e.g.
        ``Trainer.averaged``) in place of the model's own weights from the next ``run()`` on; None goes
        back to the model's.  The vector is read at ``run()``, so one that keeps being updated is scored
        as it stands then.  Returns self: ``Evaluator(model, ds, B).use_params(tr.averaged).run()``."""
        if params is not None and self.engines:
            self.engines[0][0]._params_ptr(params)          # shape, dtype, device, alignment
        self.params = params
        return self

    def _enqueue(self) -> None:
        """The whole pass on the current stream: packs, forwards, one metrics call.  No host sync."""
        from .ops import eval_metrics
        done = 0
        for eng, X, ln in self.engines:
            b = eng.cfg.B
            while done + b <= self.n_local:
                kw = dict(lengths_out=ln) if ln is not None else {}
                self.ds.batch(self.idx[done:done + b], out=X,
                              labels_out=self.labels[done:done + b], **kw)
                eng.forward(X, ln, out=self.logits[done:done + b], params=self.params)
                done += b
        assert done == self.n_local
        self.acc.zero_()
        if self.n_local:
            eval_metrics(self.logits, self.labels, self.topk, self.counts, 0, self.confusion,
                         self.loss_sum)

    @torch.no_grad()
    def run(self) -> dict:
        """{"loss": per-sample mean, "acc", "topk_acc", "n": rows scored, "n_skipped",
        "per_class_acc": float64 [C] (NaN for a class without rows), "confusion": int64 [C, C]
        indexed [label, prediction]}, summed over the ranks.  One host read."""
        self._enqueue()
        if self.world > 1:
            dist.all_reduce(self.acc[:-1], group=self.pg)
            dist.all_reduce(self.loss_sum, group=self.pg)
        host = self.acc.cpu()
        scored, top1, topk, skipped = (int(v) for v in host[:4])
        conf = host[4:-1].view(self.C, self.C).clone()
        loss_sum = float(host[-1:].view(torch.float64)[0])
        per_class = conf.diagonal().double() / conf.sum(1).double()
        d = max(scored, 1)
        return dict(loss=loss_sum / d, acc=top1 / d, topk_acc=topk / d, n=scored, n_skipped=skipped,
                    per_class_acc=per_class, confusion=conf)
