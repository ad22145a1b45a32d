"""CPU half of the solver (fusiontransformer_amd/optim.py, trainer.build_optimizer / build_scheduler, csrc/ftx_optim.hip's argument
checks): on CPU parameters the own optimizers ARE their torch parents, with max_grad_norm they are clip_grad_norm_ + parent; the
float64 restatements of tests/optim_ref.py are pinned to torch's float64 optimizers; the builders pass the config through; the
schedulers follow their closed forms; the new entries are in the binding table and refuse bad arguments before any launch."""
import math
import warnings

import numpy as np
import pytest
import torch

from tests import optim_ref as R
from tests import solver_cases as S

SMALL = [(1,), (257,), (33, 7), (5,), (3, 8, 6)]       # tensor 4 skips steps 1-2, as in the device tests


def _small_inputs(seed=5, steps=4):
    return S.inputs(seed, SMALL, steps)


OWN = [("SGD", dict(momentum=0.9, dampening=0.1)), ("SGD", dict(momentum=0.9, nesterov=True)), ("SGD", dict()), ("AdamW", dict()),
       ("Adam", dict())]


@pytest.mark.parametrize("rule,kwargs", OWN)
@pytest.mark.parametrize("max_norm", [None, 3.0])
def test_on_cpu_parameters_the_own_optimizers_are_their_parents(rule, kwargs, max_norm):
    from fusiontransformer_amd import optim
    base, grads = _small_inputs()
    pa, pb = S.make_params(base, "cpu", awkward=False), S.make_params(base, "cpu", awkward=False)
    own = getattr(optim, rule)(pa, lr=S.LR, weight_decay=S.WD, max_grad_norm=max_norm, **kwargs)
    ref = getattr(torch.optim, rule)(pb, lr=S.LR, weight_decay=S.WD, **kwargs)
    assert isinstance(own, getattr(torch.optim, rule))
    for g in grads:
        S.set_grads(pa, g, "cpu", awkward=False)
        S.set_grads(pb, g, "cpu", awkward=False)
        if max_norm is not None:
            norm = torch.nn.utils.clip_grad_norm_([p for p in pb if p.grad is not None], max_norm)
        own.step()
        ref.step()
        if max_norm is not None:
            assert torch.equal(own.last_grad_norm, norm)
            assert torch.equal(own.last_clip_coef, torch.clamp(max_norm / (norm + 1e-6), max=1.0))
            assert float(own.last_clip_coef) < 1.0
        else:
            assert own.last_grad_norm is None and own.last_clip_coef is None
        for a, b in zip(pa, pb):
            assert torch.equal(a, b)
    sa, sb = own.state_dict(), ref.state_dict()
    assert sa["state"].keys() == sb["state"].keys()
    for i in sb["state"]:
        assert sa["state"][i].keys() == sb["state"][i].keys()
        for k, v in sb["state"][i].items():
            assert torch.equal(torch.as_tensor(sa["state"][i][k]), torch.as_tensor(v)), (i, k)


def test_max_grad_norm_must_be_positive():
    from fusiontransformer_amd import optim
    p = [torch.nn.Parameter(torch.zeros(3))]
    for cls in (optim.Adam, optim.AdamW, optim.SGD):
        with pytest.raises(ValueError):
            cls(p, max_grad_norm=0.0)
        with pytest.raises(ValueError):
            cls(p, max_grad_norm=float("nan"))


RULES64 = [("SGD", dict(momentum=0.9)), ("SGD", dict(momentum=0.9, nesterov=True)), ("SGD", dict(momentum=0.9, dampening=0.1)),
           ("SGD", dict(momentum=0.0)), ("AdamW", dict()), ("Adam", dict())]


@pytest.mark.parametrize("rule,kwargs", RULES64)
@pytest.mark.parametrize("clipped", [False, True])
def test_restatements_agree_with_torch_in_float64(rule, kwargs, clipped):
    base, grads = _small_inputs(seed=9, steps=5)
    max_norm = S.max_norm_for(grads) if clipped else None
    params = S.make_params(base, "cpu", torch.float64, awkward=False)
    opt = getattr(torch.optim, rule)(params, lr=S.LR, weight_decay=S.WD, foreach=False, **kwargs)
    shots = S.drive(opt, params, grads, S.STATE_KEYS[rule], "cpu", torch.float64, clip=max_norm, awkward=False)
    refs = S.reference(rule, kwargs, base, grads, max_norm)
    for shot, ref in zip(shots, refs):
        for k in shot:
            for a, b in zip(shot[k], ref.get(k, [None] * len(shot[k]))):
                assert (a is None) == (b is None), k
                if a is not None:
                    np.testing.assert_allclose(b, a, rtol=1e-12, atol=0, err_msg=k)


def test_restated_clip_is_clip_grad_norm():
    _, grads = _small_inputs(seed=11, steps=1)
    for max_norm, below in ((1.0, False), (1e6, True)):
        ts = [torch.nn.Parameter(torch.zeros(g.shape, dtype=torch.float64)) for g in grads[0]]
        for t, g in zip(ts, grads[0]):
            t.grad = torch.from_numpy(g).double()
        norm = torch.nn.utils.clip_grad_norm_(ts, max_norm)
        ref_norm, coef, scaled = R.clip(grads[0], max_norm)
        assert abs(float(norm) - ref_norm) <= 1e-12 * ref_norm and (coef == 1.0) == below
        for t, s in zip(ts, scaled):
            np.testing.assert_allclose(s, t.grad.numpy(), rtol=1e-12, atol=0)
    assert R.clip([np.array([1.0, np.inf], np.float32)], 1.0)[:2] == (math.inf, 0.0)
    n, c, _ = R.clip([np.array([1.0, np.nan], np.float32)], 1.0)
    assert math.isnan(n) and math.isnan(c)
    assert R.coef_f32(np.float32(np.inf), 1.0) == 0.0 and np.isnan(R.coef_f32(np.float32(np.nan), 1.0)) and R.coef_f32(np.float32(0.0), 1.0) == 1.0


# ---------------------------------------------------------------------------------------------------------------- builders
def _toy():
    return torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.Linear(3, 2))


def test_build_optimizer_passes_the_type_node_through():
    from fusiontransformer_amd import config, optim
    from fusiontransformer_amd.trainer import build_optimizer
    cfg = config.get_cfg_defaults()
    assert cfg.OPTIMIZER.SGD.momentum == 0.9 and cfg.OPTIMIZER.SGD.dampening == 0.0
    assert cfg.OPTIMIZER.MAX_GRAD_NORM == 0.0 and cfg.OPTIMIZER.native is False
    cfg.OPTIMIZER.TYPE = "Adam"
    cfg.OPTIMIZER.Adam.betas = (0.8, 0.95)
    opt = build_optimizer(cfg, _toy())
    assert type(opt) is torch.optim.Adam and opt.defaults["betas"] == (0.8, 0.95)       # CPU parameters, no clipping: as before
    cfg.OPTIMIZER.TYPE = "SGD"
    cfg.OPTIMIZER.SGD.momentum = 0.7
    opt = build_optimizer(cfg, _toy())
    assert type(opt) is torch.optim.SGD and opt.defaults["momentum"] == 0.7 and opt.defaults["lr"] == cfg.OPTIMIZER.BASE_LR
    cfg.OPTIMIZER.TYPE = "AdamW"
    assert type(build_optimizer(cfg, _toy())) is torch.optim.AdamW
    cfg.OPTIMIZER.TYPE = "RMSprop"
    assert type(build_optimizer(cfg, _toy())) is torch.optim.RMSprop
    # native / MAX_GRAD_NORM
    cfg.OPTIMIZER.TYPE, cfg.OPTIMIZER.native = "SGD", True
    opt = build_optimizer(cfg, _toy())
    assert type(opt) is optim.SGD and opt.max_grad_norm is None and opt.defaults["momentum"] == 0.7
    cfg.OPTIMIZER.native, cfg.OPTIMIZER.MAX_GRAD_NORM = False, 2.5
    for typ, cls in (("SGD", optim.SGD), ("AdamW", optim.AdamW), ("Adam", optim.Adam)):
        cfg.OPTIMIZER.TYPE = typ
        opt = build_optimizer(cfg, _toy())
        assert type(opt) is cls and opt.max_grad_norm == 2.5
    cfg.OPTIMIZER.TYPE = "RMSprop"
    with pytest.raises(ValueError):
        build_optimizer(cfg, _toy())


def test_multistep_scheduler_follows_the_closed_form():
    from fusiontransformer_amd import config
    from fusiontransformer_amd.trainer import build_scheduler
    cfg = config.get_cfg_defaults()
    assert cfg.SCHEDULER.TYPE == "" and cfg.SCHEDULER.MAX_EPOCH == 1 and cfg.SCHEDULER.CLIP_LR == 0.0
    assert cfg.SCHEDULER.StepLR.gamma == 0.1 and tuple(cfg.SCHEDULER.MultiStepLR.milestones) == ()
    opt = torch.optim.SGD(_toy().parameters(), lr=0.5)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        assert build_scheduler(cfg, opt) is None
    assert any("No scheduler" in str(w.message) for w in seen)
    cfg.SCHEDULER.TYPE = "MultiStepLR"
    cfg.SCHEDULER.MultiStepLR.milestones, cfg.SCHEDULER.MultiStepLR.gamma = (3, 5), 0.1
    sch = build_scheduler(cfg, opt)
    assert isinstance(sch, torch.optim.lr_scheduler.MultiStepLR)
    for step in range(7):
        want = 0.5 * 0.1 ** ((step >= 3) + (step >= 5))
        assert math.isclose(opt.param_groups[0]["lr"], want, rel_tol=1e-12), step
        opt.step()
        sch.step()
    cfg.SCHEDULER.TYPE = "NoSuchLR"
    with pytest.raises(ValueError):
        build_scheduler(cfg, opt)


def test_clip_lr_clips_what_it_reports_and_nothing_else():
    from fusiontransformer_amd import config
    from fusiontransformer_amd.trainer import ClipLR, build_scheduler
    cfg = config.get_cfg_defaults()
    cfg.SCHEDULER.TYPE, cfg.SCHEDULER.CLIP_LR = "MultiStepLR", 0.02
    cfg.SCHEDULER.MultiStepLR.milestones = (1, 2)
    opt = torch.optim.SGD(_toy().parameters(), lr=0.5)
    sch = build_scheduler(cfg, opt)
    assert isinstance(sch, ClipLR) and sch.min_lr == 0.02 and sch.last_epoch == 0
    inner = sch.scheduler
    for step in range(4):
        lr = 0.5 * 0.1 ** min(step, 2)
        assert math.isclose(opt.param_groups[0]["lr"], lr, rel_tol=1e-12)          # the optimizer follows the inner scheduler ...
        assert math.isclose(inner.get_last_lr()[0], lr, rel_tol=1e-12)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                                        # get_lr() outside step() warns in torch
            assert sch.get_lr() == [max(0.02, x) for x in inner.get_lr()]          # ... ClipLR clips what get_lr() reports
        opt.step()
        sch.step()
    assert opt.param_groups[0]["lr"] < 0.02 and inner.last_epoch == 4
    with pytest.raises(TypeError):
        ClipLR(object())


def test_warmup_multistep_matches_its_formula():
    from fusiontransformer_amd import config
    from fusiontransformer_amd.trainer import WarmupMultiStepLR, build_scheduler
    opt = torch.optim.SGD(_toy().parameters(), lr=0.2)
    cfg = config.get_cfg_defaults()
    cfg.SCHEDULER.TYPE = "WarmupMultiStepLR"
    cfg.SCHEDULER.WarmupMultiStepLR = {"milestones": (4, 6), "gamma": 0.5, "warmup_factor": 0.25, "warmup_steps": 3}
    sch = build_scheduler(cfg, opt)
    assert isinstance(sch, WarmupMultiStepLR)
    for step in range(8):
        alpha = step / 3
        warm = 0.25 * (1 - alpha) + alpha if step < 3 else 1.0        # step 3 is the first one past the warm-up
        want = 0.2 * warm * 0.5 ** ((step >= 4) + (step >= 6))
        assert math.isclose(opt.param_groups[0]["lr"], want, rel_tol=1e-12), step
        opt.step()
        sch.step()
    const = WarmupMultiStepLR(torch.optim.SGD(_toy().parameters(), lr=1.0), (2,), warmup_factor=0.1, warmup_steps=2, warmup_method="constant")
    assert math.isclose(const.get_last_lr()[0], 0.1)
    with pytest.raises(ValueError):
        WarmupMultiStepLR(opt, (3, 2))
    with pytest.raises(ValueError):
        WarmupMultiStepLR(opt, (2, 3), warmup_method="cosine")


class _OneHead(torch.nn.Module):
    """A model whose only output is one logits tensor, its own parameter (the toy of tests/test_single_modality_host.py)."""

    def __init__(self, logits):
        super().__init__()
        self.head = torch.nn.Parameter(torch.from_numpy(logits.copy()))

    def forward(self, batch):
        return {"lidar_seg_logit": 1.0 * self.head}


def test_train_step_advances_the_scheduler_once_per_step():
    from fusiontransformer_amd import config
    from fusiontransformer_amd.trainer import TrainStep, build_scheduler
    rng = np.random.default_rng(2)
    model = _OneHead(rng.standard_normal((50, 20)).astype(np.float32))
    label = torch.from_numpy(rng.integers(0, 20, 50))
    cfg = config.lidar_cfg()
    cfg.OPTIMIZER.TYPE, cfg.OPTIMIZER.BASE_LR = "SGD", 0.5
    cfg.SCHEDULER.TYPE = "MultiStepLR"
    cfg.SCHEDULER.MultiStepLR.milestones = (2,)
    step = TrainStep(cfg, model)
    assert step.scheduler is None                                                   # the default changes nothing
    step.scheduler = None
    sch = build_scheduler(cfg, step.optimizer)
    step = TrainStep(cfg, model, optimizer=step.optimizer, scheduler=sch)
    rates = []
    for _ in range(4):
        rates.append(step.optimizer.param_groups[0]["lr"])
        step({"seg_label": label})
    assert sch.last_epoch == 4
    np.testing.assert_allclose(rates, [0.5, 0.5, 0.05, 0.05], rtol=1e-12)


# ---------------------------------------------------------------------------------------------------------------- C ABI
NEW = ("ftx_adam_step_scaled", "ftx_adamw_step", "ftx_sgd_step", "ftx_grad_sumsq", "ftx_grad_norm_finalize")


def test_new_entries_are_bound_and_refuse_bad_arguments_before_any_launch(ftx_lib):
    from fusiontransformer_amd import _lib
    from fusiontransformer_amd.optim import _REC, _REC_SGD
    from tests.nolaunch import NoLaunch
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(ftx_lib, name), name
        with pytest.raises(AssertionError):
            getattr(NoLaunch(), name)()                                             # a launching entry, not a host-only query
    L = ftx_lib
    assert NoLaunch().ftx_adam_chunk_elements() == 16384                            # the host-only queries answer without a GPU
    assert NoLaunch().ftx_adam_tensor_bytes() == _REC.itemsize == _REC_SGD.itemsize == 48
    assert [_REC_SGD.fields[k][1] for k in ("p", "g", "n")] == [_REC.fields[k][1] for k in ("p", "g", "n")]
    # empty work is a no-op, a negative count and a null table are errors
    assert L.ftx_adam_step_scaled(0, 0, 0, 0, 0.9, 0.999, 1e-8, 0.0, 0, None) == 0
    assert L.ftx_adamw_step(0, 0, 0, 0, 0.9, 0.999, 1e-8, 1e-3, 1e-2, 0, None) == 0
    assert L.ftx_sgd_step(0, 0, 0, 0, 1e-3, 0.9, 0.0, 0.0, 0, 0, None) == 0
    assert L.ftx_grad_sumsq(0, 0, 0, 0, 0, None) == 0
    for rc in (L.ftx_adam_step_scaled(0, 0, 0, -1, 0.9, 0.999, 1e-8, 0.0, 0, None), L.ftx_adamw_step(0, 0, 0, -1, 0.9, 0.999, 1e-8, 1e-3, 1e-2, 0, None),
               L.ftx_sgd_step(0, 0, 0, -1, 1e-3, 0.9, 0.0, 0.0, 0, 0, None), L.ftx_grad_sumsq(0, 0, 0, -1, 0, None),
               L.ftx_grad_norm_finalize(0, -1, 1.0, 16, None)):
        assert rc != 0 and b"< 0" in L.ftx_last_error()
    for rc in (L.ftx_adam_step_scaled(0, 0, 0, 1, 0.9, 0.999, 1e-8, 0.0, 0, None), L.ftx_adamw_step(0, 0, 0, 1, 0.9, 0.999, 1e-8, 1e-3, 1e-2, 0, None),
               L.ftx_sgd_step(0, 0, 0, 1, 1e-3, 0.9, 0.0, 0.0, 0, 0, None), L.ftx_grad_sumsq(0, 0, 0, 1, 0, None),
               L.ftx_grad_sumsq(16, 16, 16, 1, 0, None), L.ftx_grad_norm_finalize(0, 1, 1.0, 16, None), L.ftx_grad_norm_finalize(16, 1, 1.0, 0, None)):
        assert rc != 0 and b"null" in L.ftx_last_error()
    # hyper-parameters out of range
    bad = [L.ftx_adam_step_scaled(16, 16, 16, 1, 1.0, 0.999, 1e-8, 0.0, 0, None), L.ftx_adamw_step(16, 16, 16, 1, 0.9, 1.0, 1e-8, 1e-3, 1e-2, 0, None),
           L.ftx_adamw_step(16, 16, 16, 1, 0.9, 0.999, 1e-8, -1e-3, 1e-2, 0, None), L.ftx_adamw_step(16, 16, 16, 1, 0.9, 0.999, 1e-8, 1e-3, -1e-2, 0, None),
           L.ftx_sgd_step(16, 16, 16, 1, -1e-3, 0.9, 0.0, 0.0, 0, 0, None), L.ftx_sgd_step(16, 16, 16, 1, 1e-3, -0.9, 0.0, 0.0, 0, 0, None),
           L.ftx_sgd_step(16, 16, 16, 1, 1e-3, 0.9, 0.0, -1.0, 0, 0, None), L.ftx_sgd_step(16, 16, 16, 1, 1e-3, 0.9, float("nan"), 0.0, 0, 0, None)]
    assert all(rc != 0 for rc in bad) and b"hyper-parameter" in L.ftx_last_error()
    assert L.ftx_sgd_step(16, 16, 16, 1, 1e-3, 0.0, 0.0, 0.0, 1, 0, None) != 0 and b"nesterov" in L.ftx_last_error()
    assert L.ftx_sgd_step(16, 16, 16, 1, 1e-3, 0.9, 0.1, 0.0, 1, 0, None) != 0 and b"nesterov" in L.ftx_last_error()
    for max_norm in (0.0, -1.0, float("nan")):
        assert L.ftx_grad_norm_finalize(16, 1, max_norm, 16, None) != 0 and b"max_norm" in L.ftx_last_error()
