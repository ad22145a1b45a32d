"""Train step: the counterpart of SemanticTrainer.train_step
(FusionTransformer/modules/SemanticTrainer.py:141-209), for the fusion models and for the LiDAR-only and
image-only baselines it branches to (SemanticTrainer.py:157-200, SemanticTorchpackTrainer.py:70-106).

Fusion path:

Same loss: weighted CE x2 + lambda_xm * KL x2 in the additive form of
SemanticTrainer.py:158-178, Adam step.  Differences, all behaviour-preserving:
  * one backward of (loss_2d + loss_3d) instead of two backward calls: the image features enter
    the LiDAR branch detached (middle_fusion.py:102), so the two loss graphs are disjoint and
    the summed gradients are identical;
  * no `.item()` / `.cpu()` host syncs inside the step (the reference has 4+ per step);
    losses and the IoU confusion matrices stay on the device.
Single-modality paths (cfg.MODEL.USE_LIDAR / USE_IMAGE without USE_FUSION): one weighted CE on the one head the model has
(`functional.seg_loss`), one backward; lambda_xm and DUAL_HEAD play no part (SemanticTrainer.py:180-186)."""
from __future__ import annotations

import torch
import torch.nn.functional as F


def default_class_weights(num_classes, device=None):
    """The torchpack trainer's fallback when cfg.TRAIN.CLASS_WEIGHTS is empty (SemanticTorchpackTrainer.py:28-32): ones, class 0 ignored."""
    w = torch.ones(num_classes, device=device)
    w[0] = 0
    return w


def fusion_losses(preds, seg_label, class_weights, lambda_xm, dual_head, mix="additive"):
    """(loss_2d, loss_3d) exactly as SemanticTrainer.py:158-178 (mix="additive") or as the torchpack / DDP trainer's
    calc_loss, SemanticTorchpackTrainer.py:70-106 (mix="torchpack": (1-lambda)*CE + lambda*KL)."""
    seg_label = seg_label.long()
    loss_3d = F.cross_entropy(preds["lidar_seg_logit"], seg_label, weight=class_weights)
    loss_2d = F.cross_entropy(preds["img_seg_logit"], seg_label, weight=class_weights)
    if lambda_xm > 0:
        seg_logit_2d = preds["img_seg_logit2"] if dual_head else preds["img_seg_logit"]
        seg_logit_3d = preds["lidar_seg_logit2"] if dual_head else preds["lidar_seg_logit"]
        xm_loss_2d = F.kl_div(F.log_softmax(seg_logit_2d, dim=1), F.softmax(preds["lidar_seg_logit"].detach(), dim=1),
                              reduction="none").sum(1).mean()
        xm_loss_3d = F.kl_div(F.log_softmax(seg_logit_3d, dim=1), F.softmax(preds["img_seg_logit"].detach(), dim=1),
                              reduction="none").sum(1).mean()
        if mix == "torchpack":
            loss_2d = (1 - lambda_xm) * loss_2d + lambda_xm * xm_loss_2d
            loss_3d = (1 - lambda_xm) * loss_3d + lambda_xm * xm_loss_3d
        else:
            loss_2d = loss_2d + lambda_xm * xm_loss_2d
            loss_3d = loss_3d + lambda_xm * xm_loss_3d
    return loss_2d, loss_3d


def build_optimizer(cfg, model):
    """common/solver/build.py:7-20: getattr(torch.optim, TYPE)(params, lr, weight_decay, **cfg.OPTIMIZER.<TYPE>).

    On the GPU "Adam" is fusiontransformer_amd.optim.Adam (torch.optim.Adam's rule and state layout, one libftx launch), and
    cfg.OPTIMIZER.native routes "SGD" and "AdamW" to the package's own classes too.  cfg.OPTIMIZER.MAX_GRAD_NORM > 0 asks for max-norm
    gradient clipping fused into the step (optim.py): it implies `native` for those two and is an error for every other TYPE."""
    opt = cfg.OPTIMIZER
    params = [p for p in model.parameters() if p.requires_grad]
    kwargs = dict(lr=opt.BASE_LR, weight_decay=opt.WEIGHT_DECAY, **dict(opt.get(opt.TYPE) or {}))
    max_norm = float(opt.get("MAX_GRAD_NORM", 0.0) or 0.0)
    on_gpu = bool(params) and params[0].is_cuda
    own = opt.TYPE == "Adam" and (on_gpu or max_norm > 0) or opt.TYPE in ("SGD", "AdamW") and (bool(opt.get("native", False)) or max_norm > 0)
    if max_norm > 0 and not own:
        raise ValueError("OPTIMIZER.MAX_GRAD_NORM is supported for TYPE 'Adam', 'AdamW' and 'SGD', not for %r" % (opt.TYPE,))
    if own:
        from . import optim      # torch.optim's rules and state layouts, stepped by one libftx launch each (csrc/ftx_optim.hip)
        if max_norm > 0:
            kwargs["max_grad_norm"] = max_norm
        return getattr(optim, opt.TYPE)(params, **kwargs)
    if opt.TYPE == "AdamW" and on_gpu:
        kwargs.setdefault("fused", True)  # same update rule, one multi-tensor kernel instead of ~10 passes over 108 M parameters
    return getattr(torch.optim, opt.TYPE)(params, **kwargs)


class WarmupMultiStepLR(torch.optim.lr_scheduler.LRScheduler):
    """common/solver/lr_scheduler.py:6-50: MultiStepLR behind a warm-up.  While last_epoch < warmup_steps the rate is multiplied by
    warmup_factor ("constant") or by the line from warmup_factor at step 0 to 1 at warmup_steps ("linear"); throughout,
    lr = base_lr * warm-up * gamma ** (number of milestones <= last_epoch)."""

    def __init__(self, optimizer, milestones, gamma=0.1, warmup_factor=0.1, warmup_steps=1, warmup_method="linear", last_epoch=-1):
        if list(milestones) != sorted(milestones):
            raise ValueError("milestones must be increasing, got %r" % (milestones,))
        if warmup_method not in ("constant", "linear"):
            raise ValueError("warmup_method must be 'constant' or 'linear', got %r" % (warmup_method,))
        self.milestones, self.gamma = list(milestones), gamma
        self.warmup_factor, self.warmup_steps, self.warmup_method = warmup_factor, warmup_steps, warmup_method
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        import bisect
        warm = 1
        if self.last_epoch < self.warmup_steps:
            if self.warmup_method == "constant":
                warm = self.warmup_factor
            else:
                alpha = float(self.last_epoch) / self.warmup_steps
                warm = self.warmup_factor * (1 - alpha) + alpha
        decay = self.gamma ** bisect.bisect_right(self.milestones, self.last_epoch)
        return [base * warm * decay for base in self.base_lrs]


class ClipLR:
    """common/solver/lr_scheduler.py:53-75, kept faithful: what `get_lr()` REPORTS is max(min_lr, lr); everything else -- `step()`,
    `state_dict()`, `last_epoch`, ... -- is the wrapped scheduler's.  So the optimizer's own rate follows the wrapped scheduler and is
    NOT clipped; a caller who wants the rate itself bounded has to bound it in the scheduler."""

    def __init__(self, scheduler, min_lr=1e-5):
        if not isinstance(scheduler, torch.optim.lr_scheduler.LRScheduler):
            raise TypeError("ClipLR wraps a torch.optim.lr_scheduler.LRScheduler")
        self.scheduler = scheduler
        self.min_lr = min_lr

    def get_lr(self):
        return [max(self.min_lr, lr) for lr in self.scheduler.get_lr()]

    def __getattr__(self, name):
        if name == "scheduler":      # not set yet (unpickling): nothing to forward to
            raise AttributeError(name)
        return getattr(self.scheduler, name)


def build_scheduler(cfg, optimizer):
    """common/solver/build.py:23-41: '' builds nothing (with a warning); a name in torch.optim.lr_scheduler is built with
    cfg.SCHEDULER.<TYPE> as keyword arguments, so is this module's WarmupMultiStepLR; CLIP_LR > 0 wraps the result in ClipLR."""
    import warnings
    sch = cfg.SCHEDULER
    name = sch.TYPE
    if name == "":
        warnings.warn("No scheduler is built.")
        return None
    kind = WarmupMultiStepLR if name == "WarmupMultiStepLR" else getattr(torch.optim.lr_scheduler, name, None)
    if kind is None:
        raise ValueError("Unsupported type of scheduler: %r" % (name,))
    scheduler = kind(optimizer, **dict(sch.get(name) or {}))
    if sch.get("CLIP_LR", 0.0) > 0.0:
        scheduler = ClipLR(scheduler, min_lr=sch.CLIP_LR)
    return scheduler


class TrainStep:
    def __init__(self, cfg, model, optimizer=None, metrics=None, grad_reducer=None, loss_mix="additive", scheduler=None):
        """loss_mix="additive": SemanticTrainer.train_step (the single-process trainer); "torchpack": the DDP trainer's mix and its
        default class weights (SemanticTorchpackTrainer.py:28-32,70-106) -- the one BASELINE configs[3] / [4] follow.
        scheduler (build_scheduler's result, optional): stepped once per training step, after the optimizer -- the reference's
        per-iteration placement (SemanticTrainer.py:202-217)."""
        if loss_mix not in ("additive", "torchpack"):
            raise ValueError("loss_mix must be 'additive' or 'torchpack'")
        self.cfg, self.model, self.loss_mix = cfg, model, loss_mix
        # the reference's order (SemanticTrainer.py:157,180,184): fusion, else LiDAR only, else image only
        m = cfg.MODEL
        self.mode = "fusion" if m.get("USE_FUSION") else "lidar" if m.get("USE_LIDAR") else "image" if m.get("USE_IMAGE") else None
        if self.mode is None:
            raise ValueError("TrainStep: cfg.MODEL sets none of USE_FUSION / USE_LIDAR / USE_IMAGE")
        self.optimizer = optimizer if optimizer is not None else build_optimizer(cfg, model)
        dev = next(model.parameters()).device
        cw = cfg.TRAIN.CLASS_WEIGHTS
        self.class_weights = torch.tensor(cw, dtype=torch.float32, device=dev) if len(cw) > 0 else None
        if self.class_weights is None and loss_mix == "torchpack":
            self.class_weights = default_class_weights(int(cfg.MODEL.NUM_CLASSES), dev)
        self.lambda_xm = float(cfg.TRAIN.FusionTransformer.lambda_xm)
        self.dual_head = bool(cfg.MODEL.DUAL_HEAD)
        if metrics is not None and hasattr(metrics, "update_dict"):
            metrics = (metrics,)       # build_model returns one bare SegIoU for the single-modality models
        self.metrics = metrics or ()
        self.grad_reducer = grad_reducer
        self.scheduler = scheduler
        self.fused_loss = True
        self.prefetch_wait = False     # next_batch: start its index build without blocking this thread (SPVCNN.prepare(wait=False))
        self.prefetch_budget_ms = 1.5  # ... then poll its host reads this long at most
        self._prefetch_misses = self._prefetch_pause = 0
        self.last = {}

    def reset_prefetch(self):
        """Forget what the self-pausing index prefetch learnt (call when the batch size or shape of the stream of batches changes)."""
        self._prefetch_misses = self._prefetch_pause = 0

    def __call__(self, data_batch, next_batch=None):
        """One training step on `data_batch`.  `next_batch` (optional): the batch of the FOLLOWING step.  Its index build (voxel sets of the
        five levels, kernel maps, point <-> voxel indices: ~230 small kernels and two host reads, models/_fusion_common.prepare_batch)
        is started on a third stream as soon as this step's backward has been issued, without blocking this thread; after the
        optimizer has been issued the build's reads are polled for at most `prefetch_budget_ms` and every part whose sizes have arrived
        is issued too; what is left is finished by the next forward.  The chain of small dependent kernels then runs BESIDE this step's
        backward instead of after it.  Same kernels and results either way (tests/test_model_gpu.py).  `prefetch_wait=True` builds
        everything with blocking reads (for a caller that owns an idle moment: a data-loading worker, an evaluation loop)."""
        ready = None
        if next_batch is not None and not self.prefetch_wait and self._prefetch_pause > 0:
            self._prefetch_pause -= 1        # the polls kept running out (large batches, see below): this step builds nothing ahead
            next_batch = None
        if next_batch is not None and torch.cuda.is_available():
            ready = torch.cuda.Event()       # whatever produced next_batch was queued before this point: its index build may start
            ready.record()                   # here and run beside this step, not behind it
        if self.grad_reducer is not None:
            self.grad_reducer.begin_step()   # zeroes the flat gradient buckets (p.grad are views into them)
        else:
            self.optimizer.zero_grad(set_to_none=True)    # first write of each gradient is a move, not fill + add
        preds = self.model(data_batch)
        if self.mode != "fusion":
            return self._single_step(preds, data_batch, next_batch, ready)
        logits = preds["lidar_seg_logit"]
        c = logits.shape[1]
        # the kernel counts one C x C matrix per head under one ignore index: metrics of another size or with differing ignore
        # indices are updated by the host path
        fits = all(m.num_classes == c for m in self.metrics) and len({m.ignore_index for m in self.metrics}) <= 1
        if self.fused_loss and fits and logits.is_cuda and c % 4 == 0 and c <= 32:
            # one fused pass: CE x2 + KL x2 + their gradients + both SegIoU confusion matrices (libftx)
            ignore_index = self.metrics[0].ignore_index if self.metrics else 0
            conf = {"3d": None, "2d": None}
            for m in self.metrics:
                if m.mat is None:
                    m.mat = torch.zeros((m.num_classes, m.num_classes), dtype=torch.int64, device=logits.device)
                conf["3d" if "3d" in m.name else "2d"] = m.mat
            from . import functional as spf
            loss_2d, loss_3d = spf.fusion_loss(preds, data_batch["seg_label"], self.class_weights, self.lambda_xm, self.dual_head,
                                               conf3d=conf["3d"], conf2d=conf["2d"], ignore_index=ignore_index, mix=self.loss_mix)
        else:
            loss_2d, loss_3d = fusion_losses(preds, data_batch["seg_label"], self.class_weights, self.lambda_xm, self.dual_head, self.loss_mix)
            with torch.no_grad():
                for m in self.metrics:
                    m.update_dict(preds, data_batch)
        (loss_2d + loss_3d).backward()
        self._finish_step(next_batch, ready)
        self.last = {"loss_2d": loss_2d.detach(), "loss_3d": loss_3d.detach()}
        return preds

    def _single_step(self, preds, data_batch, next_batch, ready):
        """The LiDAR-only / image-only step: one head, one loss, one backward."""
        key, tag = ("lidar_seg_logit", "3d") if self.mode == "lidar" else ("img_seg_logit", "2d")
        logits = preds[key]
        c = logits.shape[1]
        metrics = [m for m in self.metrics if tag in m.name]     # a metric of the other modality has no head to read here
        fits = all(m.num_classes == c for m in metrics) and len(metrics) <= 1
        if self.fused_loss and fits and logits.is_cuda and c % 4 == 0 and c <= 32:
            # one fused pass: CE + its gradient + the SegIoU confusion matrix (libftx, ftx_seg_loss)
            conf = None
            for m in metrics:
                if m.mat is None:
                    m.mat = torch.zeros((m.num_classes, m.num_classes), dtype=torch.int64, device=logits.device)
                conf = m.mat
            from . import functional as spf
            loss = spf.seg_loss(logits, data_batch["seg_label"], self.class_weights, conf=conf,
                                ignore_index=metrics[0].ignore_index if metrics else 0)
        else:
            loss = F.cross_entropy(logits, data_batch["seg_label"].long(), weight=self.class_weights)
            with torch.no_grad():
                for m in metrics:
                    m.update_dict(preds, data_batch)
        loss.backward()
        if self.mode == "image":
            next_batch = None      # no LiDAR branch, no index to build ahead
        self._finish_step(next_batch, ready)
        self.last = {"loss_" + tag: loss.detach()}
        return preds

    def _finish_step(self, next_batch, ready):
        """What follows the backward in every mode: the gradient reduction, the next batch's index build, the optimizer."""
        if self.grad_reducer is not None:
            self.grad_reducer.finish()       # the remaining gradient buckets go out before anything else is issued
        if next_batch is not None:
            from .models._fusion_common import prepare_batch
            prepare_batch(self.model, next_batch, ready=ready, wait=self.prefetch_wait)
        self.optimizer.step()
        if self.scheduler is not None:
            self.scheduler.step()
        if next_batch is not None and not self.prefetch_wait:
            # Small batches: the build's host reads arrive within a fraction of a millisecond, so a short bounded poll gets the whole
            # build issued before the next forward starts (batch 1: 14.9 -> 13.8 ms per step).  Large batches: they do not -- the small
            # index kernels sit behind the backward's big ones -- and both the poll (batch 4: +1.1 ms) and the early start (+0.3 ms)
            # cost more than they give: after two polls in a row that ran out, the next 256 steps build their index inside their own
            # forward, then the prefetch is tried again.
            from .models._fusion_common import advance_prepared
            complete = advance_prepared(next_batch, self.prefetch_budget_ms)
            self._prefetch_misses = 0 if complete else self._prefetch_misses + 1
            if self._prefetch_misses >= 2:
                self._prefetch_pause, self._prefetch_misses = 256, 0
