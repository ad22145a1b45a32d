"""CPU half of tests/test_loss_metric_gpu.py: the vectorised evaluation reference against the oracle's per-point loop, and the
strength of the loss / gradient / matrix gates (each planted mistake of a fused-loss kernel must fail them)."""
import os

import numpy as np
import pytest

from oracle import ft_oracle as O
from tests import loss_metric_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _check_eval_ref(l3, l2, inv_frames, gt_frames, n_vox, class_labels):
    (p3, p2, pe), mats = O.validate_batch(l3, l2, inv_frames, gt_frames, n_vox, class_labels)
    offs = np.concatenate([[0], np.cumsum(n_vox)[:-1]])
    inverse = np.concatenate([np.asarray(i) + o for i, o in zip(inv_frames, offs)])
    preds, rmats = R.eval_ref(l3, l2, inverse, np.concatenate(gt_frames), class_labels)
    for a, b in zip((p3, p2, pe), preds):
        assert np.array_equal(a, b)
    for a, b in zip(mats, rmats):
        assert np.array_equal(a, b)


def test_eval_reference_matches_oracle_on_golden():
    g = np.load(os.path.join(GOLDEN, "eval_scatter_back.npz"))
    nv, no = g["n_vox"], g["n_org"]
    cuts = np.cumsum(no)[:-1]
    _check_eval_ref(g["lidar_seg_logit"], g["img_seg_logit"], np.split(g["inverse_map"], cuts), np.split(g["orig_seg_label"], cuts), nv,
                    g["class_labels"])


@pytest.mark.parametrize("with_c", [True, False])
def test_eval_reference_matches_oracle_on_random_case(with_c):
    rng = np.random.default_rng(7 + with_c)
    c = 7
    labels = np.array([0, 10, 11, c if with_c else 13, 40, 252, 44])
    n_vox = np.array([50, 80, 30])
    l3 = rng.standard_normal((n_vox.sum(), c)).astype(np.float32)
    l2 = rng.standard_normal((n_vox.sum(), c)).astype(np.float32)
    l3[:5, 1] = l3[:5, 4] = 9.0                         # exact ties: first maximum
    inv = [rng.integers(0, n, 3 * n) for n in n_vox]
    gts = [rng.integers(0, c, 3 * n).astype(np.int32) for n in n_vox]
    _check_eval_ref(l3, l2, inv, gts, n_vox, labels)


def _case(rng, n=4000, c=20, scale=1.0):
    lg = R.make_logits(rng, n, c, scale, dual=True, ties=40)
    label = R.make_labels(rng, n, c, "invalid")
    return lg, label, R.spread_weights(rng, c)


@pytest.mark.parametrize("dual", [True, False])
@pytest.mark.parametrize("mix,lam", [("additive", 0.0), ("additive", 0.1), ("torchpack", 0.5)])
def test_host_restatement_passes_the_gates(dual, mix, lam):
    """The float64 restatement of the kernel agrees with the oracle's statements: the planted-mistake checks below start from
    something that passes."""
    rng = np.random.default_rng(11)
    lg, label, cw = _case(rng)
    if not dual:
        lg = {k: lg[k] for k in R.NAMES[:2]}
    cs = (1 - lam) if (mix == "torchpack" and lam > 0) else 1.0
    ref, rg = R.oracle_losses(lg, label, cw, lam, dual, mix)
    got, gg, confs = R.host_fused(lg, label, cw, lam, dual, ce_scale=cs, ignore_index=3)
    R.assert_losses_close(got, ref)
    R.assert_grads_close(gg, rg, R.logit_max(lg))
    R.assert_confs_equal(confs, (R.conf_ref(lg[R.NAMES[0]], label, 20, 3), R.conf_ref(lg[R.NAMES[1]], label, 20, 3)))


@pytest.mark.parametrize("scale", [1.0, 40.0])
@pytest.mark.parametrize("n", [4000, 65537])
@pytest.mark.parametrize("mistake", ["drop_rows", "kl_by_w", "ignore_ce_scale", "w_all_labels"])
def test_loss_and_gradient_gates_catch_planted_mistakes(mistake, n, scale):
    rng = np.random.default_rng(12)
    lg, label, cw = _case(rng, n=n, scale=scale)
    lam = 0.5
    ref, rg = R.oracle_losses(lg, label, cw, lam, True, "torchpack")
    kw = {mistake: (n % 256 or 256) if mistake == "drop_rows" else True}
    got, gg, _ = R.host_fused(lg, label, cw, lam, True, ce_scale=1 - lam, **kw)
    with pytest.raises(AssertionError):
        R.assert_losses_close(got, ref)
    with pytest.raises(AssertionError):
        R.assert_grads_close(gg, rg, R.logit_max(lg))


@pytest.mark.parametrize("mistake", ["last_max", "no_ignore"])
def test_matrix_gate_catches_planted_mistakes(mistake):
    rng = np.random.default_rng(13)
    lg, label, cw = _case(rng)
    ref = (R.conf_ref(lg[R.NAMES[0]], label, 20, 3), R.conf_ref(lg[R.NAMES[1]], label, 20, 3))
    _, _, confs = R.host_fused(lg, label, cw, 0.1, True, ignore_index=3, **{mistake: True})
    with pytest.raises(AssertionError):
        R.assert_confs_equal(confs, ref)
    for i in range(2):       # each matrix on its own
        with pytest.raises(AssertionError):
            R.assert_confs_equal(confs[i:i + 1], ref[i:i + 1])


def test_nan_gate_needs_nan_where_the_reference_has_it():
    """All labels 0 under weights with w[0] = 0: the reference's weighted mean is 0/0."""
    rng = np.random.default_rng(14)
    lg = R.make_logits(rng, 300, 20)
    label = R.make_labels(rng, 300, 20, "zeros")
    cw = np.ones(20, np.float32)
    cw[0] = 0
    ref, _ = R.oracle_losses(lg, label, cw, 0.1, True)
    assert np.isnan(ref[0]) and np.isnan(ref[1])
    got, _, _ = R.host_fused(lg, label, cw, 0.1, True)
    R.assert_losses_close(got, ref)
    with pytest.raises(AssertionError):
        R.assert_losses_close((0.5, 0.5), ref)
