"""float64 restatements of the solver's rules (csrc/ftx_optim.hip, fusiontransformer_amd/optim.py): torch.optim.SGD / Adam / AdamW and
torch.nn.utils.clip_grad_norm_.  Inputs are float32 arrays (or None for "no gradient this step"); everything is carried and returned
in float64.  tests/test_solver_host.py pins these to torch's own float64 optimizers on the CPU to 1e-12, so they restate torch and
not a reading of it; tests/test_solver_gpu.py measures the kernels and torch's float32 optimizers against them."""
import math

import numpy as np

UNIT = 2.0 ** -24


def f64(x):
    return None if x is None else np.asarray(x, dtype=np.float64)


def grad_norm(grads):
    """The exact 2-norm over every gradient that is there: squares of float32 values are exact in float64."""
    total = math.fsum(float(np.sum(f64(g).ravel() ** 2)) for g in grads if g is not None)
    return math.sqrt(total)


def clip(grads, max_norm):
    """clip_grad_norm_(error_if_nonfinite=False): (norm, coef, scaled gradients), coef = min(1, max_norm / (norm + 1e-6)); NaN stays NaN."""
    norm = grad_norm(grads)
    c = max_norm / (norm + 1e-6)
    coef = 1.0 if c > 1.0 else c
    with np.errstate(invalid="ignore"):                     # inf * 0 is the NaN clip_grad_norm_ leaves too
        return norm, coef, [None if g is None else f64(g) * coef for g in grads]


def coef_f32(norm32, max_norm):
    """The float32 formula ftx_grad_norm_finalize applies to the float32 norm it wrote."""
    with np.errstate(all="ignore"):
        c = np.float32(max_norm) / (np.float32(norm32) + np.float32(1e-6))
    return np.float32(1.0) if c > np.float32(1.0) else np.float32(c)


class SGD:
    def __init__(self, params, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, max_norm=None):
        self.p = [f64(p).copy() for p in params]
        self.buf = [None] * len(params)
        self.lr, self.momentum, self.dampening, self.weight_decay, self.nesterov, self.max_norm = lr, momentum, dampening, weight_decay, nesterov, max_norm
        self.norm = self.coef = None

    def step(self, grads, lr=None):
        lr = self.lr if lr is None else lr
        grads = [f64(g) for g in grads]
        if self.max_norm is not None:
            self.norm, self.coef, grads = clip(grads, self.max_norm)
        for i, g in enumerate(grads):
            if g is None:
                continue                                    # skipped: its "first step" stays pending
            g = g + self.weight_decay * self.p[i]
            if self.momentum != 0:
                self.buf[i] = g.copy() if self.buf[i] is None else self.momentum * self.buf[i] + (1 - self.dampening) * g
                g = g + self.momentum * self.buf[i] if self.nesterov else self.buf[i]
            self.p[i] = self.p[i] - lr * g

    def state(self):
        return {"momentum_buffer": self.buf} if self.momentum != 0 else {}


class Adam:
    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, max_norm=None):
        self.p = [f64(p).copy() for p in params]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.t = [0] * len(params)
        self.lr, self.betas, self.eps, self.weight_decay, self.decoupled, self.max_norm = lr, betas, eps, weight_decay, decoupled, max_norm
        self.norm = self.coef = None

    def step(self, grads, lr=None):
        lr = self.lr if lr is None else lr
        b1, b2 = self.betas
        grads = [f64(g) for g in grads]
        if self.max_norm is not None:
            self.norm, self.coef, grads = clip(grads, self.max_norm)
        for i, g in enumerate(grads):
            if g is None:
                continue                                    # skipped: its step counter lags
            self.t[i] += 1
            if self.decoupled:
                self.p[i] = self.p[i] * (1 - lr * self.weight_decay)
            else:
                g = g + self.weight_decay * self.p[i]
            self.m[i] = self.m[i] + (1 - b1) * (g - self.m[i])
            self.v[i] = b2 * self.v[i] + (1 - b2) * g * g
            with np.errstate(all="ignore"):
                denom = np.sqrt(self.v[i]) / math.sqrt(1 - b2 ** self.t[i]) + self.eps
                self.p[i] = self.p[i] - (lr / (1 - b1 ** self.t[i])) * (self.m[i] / denom)

    def state(self):
        return {"exp_avg": self.m, "exp_avg_sq": self.v}


def AdamW(params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=None):
    return Adam(params, lr, betas, eps, weight_decay, decoupled=True, max_norm=max_norm)


def worst_units(got, ref):
    """max |got - ref| over one tensor in units of 2^-24 times the largest magnitude of the reference tensor."""
    ref = f64(ref)
    scale = float(np.max(np.abs(ref))) if ref.size else 0.0
    err = float(np.max(np.abs(f64(got) - ref))) if ref.size else 0.0
    return 0.0 if err == 0.0 else err / (UNIT * scale)
