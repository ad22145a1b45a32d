"""Host references of the single-head segmentation loss (csrc/ftx_loss.hip, ftx_seg_loss), shared by
tests/test_single_modality_host.py (CPU) and tests/test_seg_loss_gpu.py: the float64 F.cross_entropy oracle and a float64
restatement of the kernel with switches that plant the mistakes such a kernel could make.  The gates are those of
tests/loss_metric_ref.py."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import loss_metric_ref as R


def host_seg(x, label, class_weights, ignore_index=0, drop_rows=0, w_all_labels=False, last_max=False, no_ignore=False, grad_by_n=False):
    """float64 restatement of ftx_seg_loss: loss, gradient, matrix.  The keyword switches plant one mistake each: drop_rows (the
    last rows never visited), w_all_labels (W summed over every label instead of the valid ones), last_max (argmax takes the last
    maximum), no_ignore (ignore_index not honoured), grad_by_n (the gradient normalised by n instead of W)."""
    x = np.asarray(x, dtype=np.float64)
    n, c = x.shape
    label = np.asarray(label)
    keep = np.arange(n) < n - drop_rows
    valid = (label >= 0) & (label < c)
    y = np.where(valid, label, 0)
    cw = np.ones(c) if class_weights is None else np.asarray(class_weights, dtype=np.float64)
    w = np.where(valid, cw[y], 0.0)
    W = w.sum() + (float((~valid).sum()) if w_all_labels else 0.0)
    m = x.max(1, keepdims=True)
    lp = x - (np.log(np.exp(x - m).sum(1, keepdims=True)) + m)
    oh = np.zeros((n, c))
    oh[np.arange(n), y] = valid
    with np.errstate(divide="ignore", invalid="ignore"):
        loss = -(w * lp[np.arange(n), y] * keep).sum() / W
        grad = (w / (n if grad_by_n else W))[:, None] * (np.exp(lp) - oh) * keep[:, None]
    conf = R.conf_ref(x, label, c, None if no_ignore else ignore_index, last_max, n - drop_rows)
    return loss, grad, conf


def seg_oracle(x, label, class_weights, upstream=1.0):
    """float64 F.cross_entropy autograd; labels outside [0, C) are handed over as -100, as loss_metric_ref.oracle_losses does."""
    t = torch.from_numpy(np.asarray(x, dtype=np.float64)).requires_grad_(True)
    lab = torch.from_numpy(np.asarray(label, dtype=np.int64))
    lab = torch.where((lab >= 0) & (lab < t.shape[1]), lab, torch.full_like(lab, -100))
    cw = None if class_weights is None else torch.from_numpy(np.asarray(class_weights, dtype=np.float64))
    loss = F.cross_entropy(t, lab, weight=cw)
    (upstream * loss).backward()
    return loss.item(), t.grad.numpy()
