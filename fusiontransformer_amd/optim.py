"""Adam, AdamW and SGD stepped by one libftx launch each, with max-norm gradient clipping fused in (csrc/ftx_optim.hip).

`fusiontransformer_amd.optim.Adam` is `torch.optim.Adam` -- same constructor, same update rule (L2 weight decay, no amsgrad), same
`state_dict()` layout (`step`, `exp_avg`, `exp_avg_sq` per parameter), so checkpoints move both ways -- with `step()` replaced:
the reference's `optimizer.step()` (common/solver/build.py:7-20 builds it, modules/SemanticTrainer.py steps it once per batch) walks
~300 parameter tensors; torch's fused implementation does that in 14 multi-tensor launches and ~0.9 ms of host time, this one in one
launch whose per-step host work is one pass over the gradients' addresses.  `AdamW` and `SGD` are `torch.optim.AdamW` and
`torch.optim.SGD` (momentum, dampening, nesterov, L2 weight decay; `momentum_buffer` per parameter) in the same way.

Anything the kernels do not cover (CPU parameters, non-float32, sparse gradients, amsgrad / maximize / capturable / differentiable, a
tensor learning rate; for AdamW and SGD also an explicit foreach=True / fused=True) is handed to the parent's step unchanged.

`max_grad_norm` (all three, default None = off): `torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm)` over ALL parameter groups,
fused into the step: one extra read of the gradients leaves float64 sums of squares per 16 K chunk, one block turns them into
(norm, coefficient) in device memory, and the update kernels multiply every gradient element by the coefficient as they read it.
No value crosses to the host: `optimizer.last_grad_norm` and `optimizer.last_clip_coef` are 0-dim device tensors (views of one
two-float buffer, rewritten by every step).  The one visible difference from calling clip_grad_norm_ first: `p.grad` is left UNSCALED
-- the scale is applied in flight, the gradients in memory are not rewritten.  On the fallback path step() calls clip_grad_norm_ itself
(which does rewrite p.grad) and then the parent's step, and sets the two attributes from its result."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

_REC = np.dtype([("p", "<i8"), ("m", "<i8"), ("v", "<i8"), ("g", "<i8"), ("n", "<i8"), ("step_size", "<f4"), ("inv_bc2_sqrt", "<f4")])
# the same 48 bytes as ftx_sgd_step reads them
_REC_SGD = np.dtype([("p", "<i8"), ("buf", "<i8"), ("unused", "<i8"), ("g", "<i8"), ("n", "<i8"), ("first", "<i4"), ("pad", "<i4")])


class _GroupPlan:
    """Static description of one parameter group for the kernels: the table rows and the chunk -> (tensor, offset) map."""

    def __init__(self, params, device, rec_dtype=_REC):
        L = _lib.load()
        assert int(L.ftx_adam_tensor_bytes()) == rec_dtype.itemsize
        chunk = int(L.ftx_adam_chunk_elements())
        self.params = params
        n = np.array([p.numel() for p in params], dtype=np.int64)
        per = (n + chunk - 1) // chunk
        self.n_chunks = int(per.sum())
        tid = np.repeat(np.arange(len(params), dtype=np.int32), per)
        off = np.concatenate([np.arange(k, dtype=np.int64) * chunk for k in per]) if self.n_chunks else np.zeros(0, np.int64)
        self.chunk_tensor = torch.from_numpy(tid).to(device)
        self.chunk_offset = torch.from_numpy(off).to(device)
        self.host = [torch.empty(len(params) * rec_dtype.itemsize, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        self.rec = [h.numpy().view(rec_dtype) for h in self.host]
        self.events = [None, None]
        self.turn = 0
        self.table = torch.empty(len(params) * rec_dtype.itemsize, dtype=torch.uint8, device=device)
        for r in self.rec:
            r.view(np.uint8)[:] = 0
            r["n"] = n

    def next_rec(self):
        """The pinned table to fill this step (double-buffered: the copy that last read it has been issued AND has run)."""
        k = self.turn
        self.turn ^= 1
        if self.events[k] is not None:
            self.events[k].synchronize()
        return k, self.rec[k]

    def upload(self, k):
        self.table.copy_(self.host[k], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.events[k] = ev

    def args(self):
        return self.table.data_ptr(), self.chunk_tensor.data_ptr(), self.chunk_offset.data_ptr(), self.n_chunks


class _OneLaunch:
    """What the three optimizers share: eligibility, one _GroupPlan per parameter group, the per-step table upload, the fused
    clipping and the fallback to the torch parent.  A rule supplies _covers, _new_plan, _fill and _launch."""

    def _init_native(self, max_grad_norm):
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("max_grad_norm must be positive or None")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.last_grad_norm = None
        self.last_clip_coef = None
        self._plans = {}
        self._norm_out = None
        self._partial = None

    def _drop_plans(self):
        self._plans = {}

    def _eligible(self, group):
        if group.get("maximize") or group.get("capturable") or group.get("differentiable") or not self._covers(group):
            return False
        if isinstance(group["lr"], torch.Tensor):
            return False
        dev = group["params"][0].device if group["params"] else None
        for p in group["params"]:
            if not (p.is_cuda and p.device == dev and p.dtype == torch.float32 and p.is_contiguous()):
                return False
            if p.grad is not None and (p.grad.is_sparse or p.grad.dtype != torch.float32):
                return False
        return len(group["params"]) > 0

    def _plan(self, gi, group):
        plan = self._plans.get(gi)
        params = group["params"]
        if plan is not None and len(plan.params) == len(params) and all(a is b for a, b in zip(plan.params, params)):
            return plan
        plan = self._plans[gi] = self._new_plan(list(params))
        return plan

    def _fallback_step(self, closure):
        self._drop_plans()
        self._norm_out = None      # last_grad_norm / last_clip_coef are about to be replaced by the parent path's tensors
        if self.max_grad_norm is None:
            return super().step(closure)
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        params = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
        if params:
            norm = torch.nn.utils.clip_grad_norm_(params, self.max_grad_norm)
        else:
            norm = torch.zeros(())
        self.last_grad_norm = norm
        self.last_clip_coef = torch.clamp(self.max_grad_norm / (norm + 1e-6), max=1.0)
        super().step()
        return loss

    @torch.no_grad()
    def step(self, closure=None):
        clip = self.max_grad_norm is not None
        if not all(self._eligible(g) for g in self.param_groups) or (clip and len({g["params"][0].device for g in self.param_groups}) != 1):
            return self._fallback_step(closure)      # one norm over parameters on several devices: torch's clip_grad_norm_ gathers it
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        L = _lib.load()
        plans = [self._plan(gi, group) for gi, group in enumerate(self.param_groups)]
        keep = []
        if clip:
            device = plans[0].table.device
            total = sum(plan.n_chunks for plan in plans)
            if self._norm_out is None or self._norm_out.device != device:
                self._norm_out = torch.zeros(2, dtype=torch.float32, device=device)
                self.last_grad_norm, self.last_clip_coef = self._norm_out[0], self._norm_out[1]
            if self._partial is None or self._partial.numel() != max(total, 1) or self._partial.device != device:
                self._partial = torch.empty(max(total, 1), dtype=torch.float64, device=device)
        at = 0
        for plan, group in zip(plans, self.param_groups):
            gptr = np.zeros(len(plan.params), dtype=np.int64)
            for i, p in enumerate(plan.params):
                g = p.grad
                if g is not None:
                    if not g.is_contiguous():
                        g = g.contiguous()
                        keep.append(g)
                    gptr[i] = g.data_ptr()
            k, rec = plan.next_rec()
            rec["p"] = [p.data_ptr() for p in plan.params]
            rec["g"] = gptr
            self._fill(plan, group, rec, gptr != 0)
            with torch.cuda.device(plan.table.device):
                plan.upload(k)
                if clip:
                    _lib.check(L.ftx_grad_sumsq(*plan.args(), self._partial.data_ptr() + 8 * at, _lib.stream()), "ftx_grad_sumsq")
                    at += plan.n_chunks
                else:
                    self._launch(L, plan, group, 0)
        if clip:         # the norm spans every group: all sums of squares, one finalize, then the scaled updates
            with torch.cuda.device(plans[0].table.device):
                _lib.check(L.ftx_grad_norm_finalize(self._partial.data_ptr(), at, self.max_grad_norm, self._norm_out.data_ptr(), _lib.stream()),
                           "ftx_grad_norm_finalize")
                for plan, group in zip(plans, self.param_groups):
                    self._launch(L, plan, group, self._norm_out.data_ptr() + 4)
        del keep
        return loss


class _AdamRule(_OneLaunch):
    """Adam and AdamW: one record layout, one element function; the group's decoupled_weight_decay picks the rule."""

    # ---- state_dict compatibility: the per-parameter step counters live in numpy between steps
    def _sync_steps(self):
        for plan in self._plans.values():
            for p, t in zip(plan.params, plan.steps):
                self.state[p]["step"] = torch.tensor(float(t))

    def _drop_plans(self):
        self._sync_steps()
        self._plans = {}

    def state_dict(self):
        self._sync_steps()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._plans = {}      # moments were replaced: rebuild the tables

    def _covers(self, group):
        return not group.get("amsgrad")

    def _new_plan(self, params):
        states = []
        for p in params:
            st = self.state[p]
            if len(st) == 0:     # what torch.optim.Adam._init_group creates lazily
                st["step"] = torch.tensor(0.0)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            states.append(st)
        plan = _GroupPlan(params, params[0].device)
        plan.steps = np.array([int(float(st["step"])) for st in states], dtype=np.int64)
        for r in plan.rec:
            r["m"] = [st["exp_avg"].data_ptr() for st in states]
            r["v"] = [st["exp_avg_sq"].data_ptr() for st in states]
        plan.keep = states     # the moments the table points at
        return plan

    def _fill(self, plan, group, rec, live):
        beta1, beta2 = group["betas"]
        plan.steps[live] += 1
        t = np.maximum(plan.steps, 1).astype(np.float64)
        rec["step_size"] = (float(group["lr"]) / (1.0 - beta1 ** t)).astype(np.float32)
        rec["inv_bc2_sqrt"] = (1.0 / np.sqrt(1.0 - beta2 ** t)).astype(np.float32)

    def _launch(self, L, plan, group, scale):
        beta1, beta2 = group["betas"]
        common = plan.args() + (float(beta1), float(beta2), float(group["eps"]))
        if group.get("decoupled_weight_decay"):
            _lib.check(L.ftx_adamw_step(*common, float(group["lr"]), float(group["weight_decay"]), scale, _lib.stream()), "ftx_adamw_step")
        elif scale:
            _lib.check(L.ftx_adam_step_scaled(*common, float(group["weight_decay"]), scale, _lib.stream()), "ftx_adam_step_scaled")
        else:
            _lib.check(L.ftx_adam_step(*common, float(group["weight_decay"]), _lib.stream()), "ftx_adam_step")


class Adam(_AdamRule, torch.optim.Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, *, max_grad_norm=None, **kwargs):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, **kwargs)
        self._init_native(max_grad_norm)


class AdamW(_AdamRule, torch.optim.AdamW):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, max_grad_norm=None, **kwargs):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, **kwargs)
        self._init_native(max_grad_norm)

    def _covers(self, group):
        return not (group.get("amsgrad") or group.get("foreach") or group.get("fused"))


class SGD(_OneLaunch, torch.optim.SGD):
    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, *, max_grad_norm=None, **kwargs):
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, **kwargs)
        self._init_native(max_grad_norm)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._plans = {}      # buffers were replaced: rebuild the tables

    def _covers(self, group):
        return not (group.get("foreach") or group.get("fused") or isinstance(group["weight_decay"], torch.Tensor))

    def _new_plan(self, params):
        plan = _GroupPlan(params, params[0].device, _REC_SGD)
        plan.buf = np.zeros(len(params), dtype=np.int64)
        for i, p in enumerate(params):        # a buffer that is already there (a loaded state_dict, steps of the parent) is continued
            b = self.state[p].get("momentum_buffer")
            if b is not None:
                if not (b.is_contiguous() and b.dtype == torch.float32 and b.device == p.device):
                    b = self.state[p]["momentum_buffer"] = b.to(device=p.device, dtype=torch.float32).contiguous()
                plan.buf[i] = b.data_ptr()
        return plan

    def _fill(self, plan, group, rec, live):
        first = np.zeros(len(plan.params), dtype=np.int32)
        if group["momentum"] != 0:
            for i in np.nonzero(live & (plan.buf == 0))[0]:      # torch: momentum_buffer = clone(grad) on the first step WITH a gradient
                p = plan.params[i]
                b = self.state[p]["momentum_buffer"] = torch.empty_like(p, memory_format=torch.contiguous_format)
                plan.buf[i] = b.data_ptr()
                first[i] = 1
            rec["buf"] = plan.buf
        else:
            rec["buf"] = 0
        rec["first"] = first

    def _launch(self, L, plan, group, scale):
        _lib.check(L.ftx_sgd_step(*plan.args(), float(group["lr"]), float(group["momentum"]), float(group["dampening"]),
                                  float(group["weight_decay"]), int(bool(group["nesterov"])), scale, _lib.stream()), "ftx_sgd_step")
