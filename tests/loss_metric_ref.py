"""Host references and assertion gates for the fused loss (csrc/ftx_loss.hip) and the evaluation scatter-back
(csrc/ftx_eval.hip), shared by tests/test_loss_metric_host.py (CPU) and tests/test_loss_metric_gpu.py.

* Losses and gradients: the oracle's statements (O.fusion_losses) run in float64 autograd.  Labels outside [0, C) other than
  torch's -100 are the library's extension (weight 0, not counted); they are handed to the statements as -100, which is exactly
  the masked form: cross-entropy over the valid rows, KL still averaged over all n rows.
* Confusion matrices: numpy bincount, first-maximum argmax (torch's rule), SegIoU's ignore rule.
* Evaluation: a vectorised restatement of O.validate_batch (its per-point loop is too slow at full size).
* host_fused: a float64 restatement of what the fused kernel computes, with switches that plant the mistakes a kernel could make;
  the gate-strength test checks that the gates below catch every one of them."""
import numpy as np
import torch

from oracle import ft_oracle as O

NAMES = ("lidar_seg_logit", "img_seg_logit", "lidar_seg_logit2", "img_seg_logit2")
KITTI_IDS = (10, 11, 13, 15, 16, 18, 20, 30, 31, 32, 40, 44, 48, 49, 50, 51, 52, 60, 70, 71, 72, 80, 81, 99,
             252, 253, 254, 255, 256, 257, 258, 259, 1, 2, 3, 4, 5)

LOSS_RTOL = 2e-6       # |loss - ref| <= LOSS_RTOL * max(1, |ref|)
GRAD_RTOL = 1e-4       # per element, plus grad_atol(max|logit|) * max|ref| of the tensor
GRAD_ATOL = 1e-6


def grad_atol(xmax):
    """Absolute part of the gradient gate, relative to max|ref| of the tensor: 1e-6 for logits up to 4 in magnitude, then growing
    with max|x|.  The kernel's log-probabilities are x - lse in float32, with lse within log(C) of the row maximum: each carries an
    absolute rounding error of about an ulp of max|x| (1.2e-7 * max|x|), which every probability p = exp(x - lse) takes over as a
    relative error.  A gradient element a * (p - t) with p close to its target t (1 at the label, the other head's probability in
    the KL terms) keeps that absolute error, a * 1.2e-7 * max|x| with a <= max|ref|, however small the element is.  A float32
    restatement of the kernel's arithmetic needs 0.17x / 2.0x / 7.2x the fixed 1e-6 at N(0,1) * {1, 8, 40}; this bound gives it
    1.25x / 10x / 50x.  On an MI355X (n = 300 000, dual head) the worst element used 0.13 / 0.17 / 0.12 of this bound."""
    return GRAD_ATOL * max(1.0, float(xmax) / 4.0)


# ------------------------------------------------------------------------------------------------ inputs
def make_logits(rng, n, c, scale=1.0, dual=True, ties=0):
    """float32 N(0,1)*scale logits of the four heads; the first `ties` rows of both main heads get an exactly repeated maximum
    (at two random classes), which pins the first-maximum rule of the confusion matrices."""
    out = {k: (rng.standard_normal((n, c)) * scale).astype(np.float32) for k in (NAMES if dual else NAMES[:2])}
    for k in NAMES[:2]:
        x = out[k]
        for i in range(min(ties, n)):
            a, b = rng.choice(c, 2, replace=False)
            x[i, a] = x[i, b] = x[i].max() + np.float32(0.5)
    return out


def make_labels(rng, n, c, kind="uniform"):
    if kind == "uniform":
        return rng.integers(0, c, n)
    if kind == "zero30":
        y = rng.integers(1, c, n)
        y[rng.random(n) < 0.3] = 0
        return y
    if kind == "single":
        return np.full(n, c // 2 + 1, dtype=np.int64)
    if kind == "invalid":          # some -100 (torch's ignore index) and some C / 255 / -1 (the library's extension)
        y = rng.integers(0, c, n)
        r = rng.random(n)
        y[r < 0.05] = -100
        y[(r >= 0.05) & (r < 0.07)] = c
        y[(r >= 0.07) & (r < 0.09)] = 255
        y[(r >= 0.09) & (r < 0.11)] = -1
        return y
    if kind == "zeros":
        return np.zeros(n, dtype=np.int64)
    raise ValueError(kind)


def spread_weights(rng, c):
    """Weights with several zeros and a 100x spread among the others."""
    w = (10.0 ** rng.uniform(-1, 1, c)).astype(np.float32)
    w[[0, 2, c - 1]] = 0
    return w


# ------------------------------------------------------------------------------------------------ references
def argmax_first(x):
    return np.asarray(x).argmax(1)


def conf_ref(logits, label, c, ignore_index=0, last_max=False, rows=None):
    """SegIoU's matrix of one head: rows are labels, columns the argmax; labels outside [0, C) or equal to ignore_index skipped."""
    x = np.asarray(logits)
    am = (c - 1 - x[:, ::-1].argmax(1)) if last_max else x.argmax(1)
    label = np.asarray(label)
    m = (label >= 0) & (label < c) & (label != ignore_index)
    if rows is not None:
        m &= np.arange(len(label)) < rows
    return np.bincount(label[m] * c + am[m], minlength=c * c).reshape(c, c).astype(np.int64)


def oracle_losses(logits, label, class_weights, lambda_xm, dual, mix="additive", upstream=(1.0, 1.0)):
    """(loss_2d, loss_3d) and the gradients of upstream[0]*loss_2d + upstream[1]*loss_3d with respect to every head, from the
    oracle's statements in float64 autograd.  Heads that receive no gradient come back as zeros."""
    t = {k: torch.from_numpy(np.asarray(v, dtype=np.float64)).requires_grad_(True) for k, v in logits.items()}
    lab = torch.from_numpy(np.asarray(label, dtype=np.int64))
    c = t[NAMES[0]].shape[1]
    lab = torch.where((lab >= 0) & (lab < c), lab, torch.full_like(lab, -100))
    cw = None if class_weights is None else torch.from_numpy(np.asarray(class_weights, dtype=np.float64))
    r2, r3 = O.fusion_losses(t, lab, cw, lambda_xm, dual, mix=mix)
    (upstream[0] * r2 + upstream[1] * r3).backward()
    grads = {k: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in t.items()}
    return (r2.item(), r3.item()), grads


def _log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(1, keepdims=True)
    return x - (np.log(np.exp(x - m).sum(1, keepdims=True)) + m)


def host_fused(logits, label, class_weights, lambda_xm, dual, ce_scale=1.0, ignore_index=0, drop_rows=0, kl_by_w=False,
               ignore_ce_scale=False, w_all_labels=False, last_max=False, no_ignore=False):
    """float64 restatement of ftx_fusion_loss_mix: losses, gradients of loss_2d + loss_3d, both matrices.  The keyword switches
    plant one mistake each: drop_rows (the last rows never visited), kl_by_w (KL normalised by W instead of n), ignore_ce_scale,
    w_all_labels (W summed over every label instead of the valid ones), last_max (argmax takes the last maximum), no_ignore
    (ignore_index not honoured)."""
    l3, l2 = logits[NAMES[0]], logits[NAMES[1]]
    n, c = l3.shape
    label = np.asarray(label)
    keep = (np.arange(n) < n - drop_rows)[:, None]
    valid = (label >= 0) & (label < c)
    y = np.where(valid, label, 0)
    cw = np.ones(c) if class_weights is None else np.asarray(class_weights, dtype=np.float64)
    w = np.where(valid, cw[y], 0.0)
    W = w.sum() + (float((~valid).sum()) if w_all_labels else 0.0)     # planted: invalid labels weigh 1 in W
    cs = 1.0 if ignore_ce_scale else ce_scale
    lp3, lp2 = _log_softmax(l3), _log_softmax(l2)
    p3, p2 = np.exp(lp3), np.exp(lp2)
    oh = np.zeros((n, c))
    oh[np.arange(n), y] = valid
    rows = np.arange(n)
    with np.errstate(divide="ignore", invalid="ignore"):
        ce3 = -(w * lp3[rows, y] * keep[:, 0]).sum() / W
        ce2 = -(w * lp2[rows, y] * keep[:, 0]).sum() / W
        g3 = cs * (w / W)[:, None] * (p3 - oh)
        g2 = cs * (w / W)[:, None] * (p2 - oh)
    norm = W if kl_by_w else n
    grads = {NAMES[0]: g3, NAMES[1]: g2}
    kl2 = kl3 = 0.0
    if dual:
        grads[NAMES[2]] = np.zeros((n, c))
        grads[NAMES[3]] = np.zeros((n, c))
    if lambda_xm > 0:
        q2 = _log_softmax(logits[NAMES[3]]) if dual else lp2
        q3 = _log_softmax(logits[NAMES[2]]) if dual else lp3
        kl2 = (p3 * (lp3 - q2) * keep).sum() / norm
        kl3 = (p2 * (lp2 - q3) * keep).sum() / norm
        gq2 = lambda_xm / norm * (np.exp(q2) - p3)
        gq3 = lambda_xm / norm * (np.exp(q3) - p2)
        if dual:
            grads[NAMES[3]], grads[NAMES[2]] = gq2, gq3
        else:
            grads[NAMES[1]] = g2 + gq2
            grads[NAMES[0]] = g3 + gq3
    grads = {k: v * keep for k, v in grads.items()}
    losses = (cs * ce2 + lambda_xm * kl2, cs * ce3 + lambda_xm * kl3)
    ig = None if no_ignore else ignore_index
    confs = (conf_ref(l3, label, c, ig, last_max, n - drop_rows), conf_ref(l2, label, c, ig, last_max, n - drop_rows))
    return losses, grads, confs


# ------------------------------------------------------------------------------------------------ gates
def assert_losses_close(got, ref, tol=LOSS_RTOL):
    """|loss - ref| <= tol * max(1, |ref|) for (loss_2d, loss_3d); NaN exactly where the reference is NaN."""
    for name, a, b in zip(("loss_2d", "loss_3d"), got, ref):
        a, b = float(a), float(b)
        if np.isnan(b):
            assert np.isnan(a), (name, a, b)
            continue
        assert abs(a - b) <= tol * max(1.0, abs(b)), (name, a, b, abs(a - b) / max(1.0, abs(b)))


def loss_error(got, ref):
    return max(abs(float(a) - float(b)) / max(1.0, abs(float(b))) for a, b in zip(got, ref))


def logit_max(logits):
    return max(float(np.abs(np.asarray(v)).max()) for v in logits.values())


def grad_error(got, ref, xmax=0.0):
    """Smallest multiple of the gate's bound the worst element needs: <= 1 passes."""
    worst = 0.0
    for k in ref:
        r = np.asarray(ref[k], dtype=np.float64)
        g = np.zeros_like(r) if got.get(k) is None else np.asarray(got[k], dtype=np.float64)
        bound = GRAD_RTOL * np.abs(r) + grad_atol(xmax) * np.abs(r).max()
        worst = max(worst, float((np.abs(g - r) / np.where(bound > 0, bound, 1e-300)).max()))
    return worst


def assert_grads_close(got, ref, xmax=0.0):
    """Per element |g - ref| <= 1e-4*|ref| + grad_atol(xmax)*max|ref| of that tensor (xmax: max|logit| of the inputs); heads
    without a reference gradient must come back zero (or None)."""
    for k in ref:
        r = np.asarray(ref[k], dtype=np.float64)
        g = np.zeros_like(r) if got.get(k) is None else np.asarray(got[k], dtype=np.float64)
        if not np.isfinite(r).all():
            assert np.array_equal(np.isnan(g), np.isnan(r)), k
            continue
        np.testing.assert_allclose(g, r, rtol=GRAD_RTOL, atol=grad_atol(xmax) * np.abs(r).max(), err_msg=k)


def assert_confs_equal(got, ref):
    for a, b in zip(got, ref):
        assert np.array_equal(np.asarray(a), np.asarray(b)), np.argwhere(np.asarray(a) != np.asarray(b))[:8]


# ------------------------------------------------------------------------------------------------ evaluation
def eval_ref(l3, l2, inverse, gt, class_labels):
    """Vectorised O.validate_batch on a global inverse (frame offsets already added): per original point the 3-D, 2-D and
    ensemble predictions in original ids, and the three matrices.  Entries whose inverse or gt is out of range are the library's
    extension: left out of the matrices, their predictions -1."""
    class_labels = np.asarray(class_labels, dtype=np.int64)
    c = len(class_labels)
    inverse, gt = np.asarray(inverse, dtype=np.int64), np.asarray(gt, dtype=np.int64)
    heads = [x for x in (l3, l2) if x is not None]
    n_rows = heads[0].shape[0]
    ok = (inverse >= 0) & (inverse < n_rows) & (gt >= 0) & (gt < c)
    r = np.where(ok, inverse, 0)

    def softmax(x):
        e = np.exp(x - x.max(1, keepdims=True), dtype=np.float32)
        return e / e.sum(1, keepdims=True, dtype=np.float32)

    votes = [None if l3 is None else argmax_first(l3), None if l2 is None else argmax_first(l2),
             None if (l3 is None or l2 is None) else argmax_first(softmax(np.asarray(l2, np.float32)) + softmax(np.asarray(l3, np.float32)))]
    idx_of = np.full(max(int(class_labels.max()), c) + 1, -1, dtype=np.int64)
    for i in range(c - 1, -1, -1):        # first occurrence of an id wins (the oracle's index_of)
        idx_of[class_labels[i]] = i
    gt_o = class_labels[np.where(ok, gt, 0)]
    gt_o[gt_o == 0] = c
    row = np.where(ok, idx_of[gt_o], -1)
    preds, mats = [], []
    for v in votes:
        if v is None:
            preds.append(None)
            mats.append(None)
            continue
        p = class_labels[v[r]]
        col = idx_of[p]
        m = (row >= 0) & (col >= 0)
        mats.append(np.bincount(row[m] * c + col[m], minlength=c * c).reshape(c, c).astype(np.int64))
        preds.append(np.where(ok, p, -1))
    return preds, mats
