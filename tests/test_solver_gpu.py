"""The solver on the device (csrc/ftx_optim.hip, fusiontransformer_amd/optim.py): the fused gradient norm against float64 and its
guard bands, the bit identities of the scaled Adam entry, SGD / AdamW / clipped Adam against the float64 restatements of
tests/optim_ref.py with bars taken from torch's own float32 optimizers, state_dict round trips, non-finite gradients, and one
training step through trainer.TrainStep without a host synchronisation.

Accuracy bars.  Per quantity (parameter, momentum buffer, exp_avg, exp_avg_sq) the error is the worst |x - float64| over 6 steps and
all tensors, in units of 2^-24 times the largest magnitude in the tensor.  The yardstick is torch.optim on the CPU in float32
(foreach=False, clipped variants behind clip_grad_norm_) on the same inputs; the kernel passes at no more than twice its figure: both
are correctly rounded float32 chains of equal length that differ only in where a multiply-add is contracted."""
import numpy as np
import pytest
import torch

from tests import guard as GD
from tests import optim_ref as R
from tests import solver_cases as S

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def L():
    from fusiontransformer_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _lib.load()


@pytest.fixture(scope="module")
def data():
    """(base, grads) of the awkward set, made once and never changed."""
    return S.inputs()


def call(lib, name, *args):
    """One direct call; a fault at the launch or at the synchronize ends the session."""
    from fusiontransformer_amd import _lib
    torch.cuda.synchronize()
    rc = getattr(lib, name)(*args, _lib.stream())
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("%s faulted on the GPU: %s" % (name, e), returncode=3)
    if rc == -2:
        pytest.exit("%s: %s" % (name, lib.ftx_last_error().decode("utf-8", "replace")), returncode=3)
    _lib.check(rc, name)


def tables(lib, rows, step=3, lr=S.LR, betas=(0.9, 0.999)):
    """The device table and chunk map for rows of (p, m, v, g), each a tensor or None, and the element counts."""
    from fusiontransformer_amd.optim import _REC
    chunk = int(lib.ftx_adam_chunk_elements())
    rec = np.zeros(len(rows), dtype=_REC)
    for r, (p, m, v, g, n) in zip(rec, rows):
        r["p"], r["m"], r["v"], r["g"] = (0 if t is None else t.data_ptr() for t in (p, m, v, g))
        r["n"] = n
        r["step_size"] = np.float32(lr / (1.0 - betas[0] ** step))
        r["inv_bc2_sqrt"] = np.float32(1.0 / np.sqrt(1.0 - betas[1] ** step))
    per = [-(-n // chunk) for *_, n in rows]
    tid = np.repeat(np.arange(len(rows), dtype=np.int32), per)
    off = np.concatenate([np.arange(k, dtype=np.int64) * chunk for k in per])
    return torch.from_numpy(rec.view(np.uint8).copy()).cuda(), torch.from_numpy(tid).cuda(), torch.from_numpy(off).cuda(), int(sum(per))


def fused_norm(lib, grads, max_norm, shift=0, finite=True, sizes=None):
    """ftx_grad_sumsq + ftx_grad_norm_finalize over `grads` (float32 arrays, or None: a tensor of sizes[i] elements without a
    gradient) into guarded buffers; every gradient starts `shift` elements past a 16-byte boundary.  Returns (norm, coef) as float32
    and the partials."""
    keep, rows = [], []
    for i, g in enumerate(grads):
        if g is None:
            rows.append((None, None, None, None, sizes[i]))
            continue
        whole = torch.empty(g.size + 8, dtype=F32, device="cuda")
        view = whole[4 + shift:4 + shift + g.size]
        view.copy_(torch.from_numpy(np.ascontiguousarray(g).reshape(-1)))
        assert view.data_ptr() % 16 == 4 * shift
        keep.append(whole)
        rows.append((None, None, None, view, g.size))
    table, tid, off, n_chunks = tables(lib, rows)
    pw, partial = GD.banded((n_chunks,), dtype=F64)
    ow, out = GD.banded((2,), dtype=F32)
    call(lib, "ftx_grad_sumsq", table.data_ptr(), tid.data_ptr(), off.data_ptr(), n_chunks, partial.data_ptr())
    assert GD.bands_intact(pw, partial), "ftx_grad_sumsq wrote outside partial"
    assert not finite or GD.written(partial), "ftx_grad_sumsq left an element of partial unwritten"
    call(lib, "ftx_grad_norm_finalize", partial.data_ptr(), n_chunks, max_norm, out.data_ptr())
    assert GD.bands_intact(pw, partial) and GD.bands_intact(ow, out), "ftx_grad_norm_finalize wrote outside out"
    assert not finite or GD.written(out), "ftx_grad_norm_finalize left an element of out unwritten"
    o = out.cpu().numpy()
    return o[0], o[1], partial.cpu().numpy()


def bits(x):
    return np.asarray(x).view(np.uint32 if np.asarray(x).dtype == np.float32 else np.uint64)


# ---------------------------------------------------------------------------------------------------------------- the norm
def test_norm_against_float64_and_its_bit_identities(L, data):
    base, grads = data
    max_norm, sizes = S.max_norm_for(grads), [b.size for b in base]
    for step in (0, 1):                                    # step 1: tensor 4 has no gradient, its chunks write 0.0
        g = grads[step]
        ref = R.grad_norm(g)
        norm, coef, partial = fused_norm(L, g, max_norm, sizes=sizes)
        print("ACC norm step %d: kernel %.9g float64 %.17g rel err %.3g (bar %.3g)" % (step, norm, ref, abs(float(norm) - ref) / ref, 2.0 ** -23))
        assert abs(float(norm) - ref) <= 2.0 ** -23 * ref
        assert bits(coef) == bits(R.coef_f32(norm, max_norm)) and 0.25 < coef < 0.35
        again = fused_norm(L, g, max_norm, sizes=sizes)
        assert bits(again[0]) == bits(norm) and bits(again[1]) == bits(coef) and np.array_equal(bits(again[2]), bits(partial))
        off = fused_norm(L, g, max_norm, shift=1, sizes=sizes)          # the same values one element off 16-byte alignment: the scalar path
        assert bits(off[0]) == bits(norm) and np.array_equal(bits(off[2]), bits(partial))
        if step == 1:
            chunk = int(L.ftx_adam_chunk_elements())
            first = sum(-(-n // chunk) for n in sizes[:S.SKIPS])
            assert partial[first] == 0.0 and partial[first + 1] == 0.0 and np.count_nonzero(partial) == partial.size - 2


def test_norm_over_more_partials_than_the_finalize_has_threads(L):
    g = np.random.default_rng(3).standard_normal(300 * 16384 + 3).astype(np.float32)
    ref = R.grad_norm([g])
    norm, coef, partial = fused_norm(L, [g], 1.0)
    assert partial.size == 301
    assert abs(float(norm) - ref) <= 2.0 ** -23 * ref and bits(coef) == bits(R.coef_f32(norm, 1.0))
    np.testing.assert_allclose(partial[-1], float(np.sum(g[-3:].astype(np.float64) ** 2)), rtol=1e-15)
    shifted = fused_norm(L, [g], 1.0, shift=1)
    assert bits(shifted[0]) == bits(norm) and np.array_equal(bits(shifted[2]), bits(partial))


def test_norm_without_gradients_and_below_max_norm(L, data):
    _, grads = data
    norm, coef, partial = fused_norm(L, [None, None, None], 1.0, sizes=[7, 16385, 3])
    assert norm == 0.0 and coef == 1.0 and partial.size == 4 and not partial.any()
    small = [None if g is None else g * np.float32(1e-3) for g in grads[0]]
    ref = R.grad_norm(small)
    norm, coef, _ = fused_norm(L, small, 1.0)
    assert ref < 0.5 and abs(float(norm) - ref) <= 2.0 ** -23 * ref and bits(coef) == bits(np.float32(1.0))


def test_non_finite_gradients_follow_clip_grad_norm(L):
    from fusiontransformer_amd import optim
    rng = np.random.default_rng(13)
    for bad, want in ((np.inf, (np.inf, 0.0)), (np.nan, (np.nan, np.nan))):
        base = [rng.standard_normal(n).astype(np.float32) for n in (9, 20000)]
        g = [rng.standard_normal(n).astype(np.float32) for n in (9, 20000)]
        g[1][16390] = bad
        norm, coef, _ = fused_norm(L, g, 1.0, finite=False)
        np.testing.assert_equal((float(norm), float(coef)), want)
        params = S.make_params(base, "cuda", awkward=False)
        opt = optim.Adam(params, lr=S.LR, weight_decay=S.WD, max_grad_norm=1.0)
        S.set_grads(params, g, "cuda", awkward=False)
        opt.step()
        np.testing.assert_equal((float(opt.last_grad_norm), float(opt.last_clip_coef)), want)
        ref = R.Adam(base, S.LR, weight_decay=S.WD, max_norm=1.0)
        ref.step(g)
        for p, r in zip(params, ref.p):
            got = p.detach().cpu().numpy()
            assert np.array_equal(np.isnan(got), np.isnan(r))
            np.testing.assert_allclose(got, r, rtol=2e-6, atol=2e-7, equal_nan=True)


# ---------------------------------------------------------------------------------------------------------------- bit identities
def test_scaled_adam_with_no_scale_or_one_is_ftx_adam_step(L, data):
    base, grads = data
    one = torch.ones(1, dtype=F32, device="cuda")
    runs = {}
    for form in ("ftx_adam_step", "scale NULL", "scale 1.0f"):
        st = [[S.place(b, "cuda", F32, offset=i == S.OFFSET), torch.zeros(b.shape, device="cuda"), torch.zeros(b.shape, device="cuda")] for i, b in enumerate(base)]
        for step in range(3):
            g = [None if x is None else S.place(x, "cuda", F32, offset=i == S.OFFSET) for i, x in enumerate(grads[step])]
            rows = [(p, m, v, gi, p.numel()) for (p, m, v), gi in zip(st, g)]
            table, tid, off, n_chunks = tables(L, rows, step=step + 1)
            head = (table.data_ptr(), tid.data_ptr(), off.data_ptr(), n_chunks, 0.9, 0.999, 1e-8, S.WD)
            if form == "ftx_adam_step":
                call(L, "ftx_adam_step", *head)
            else:
                call(L, "ftx_adam_step_scaled", *head, 0 if form == "scale NULL" else one.data_ptr())
        runs[form] = [t.cpu() for row in st for t in row]
    for form in ("scale NULL", "scale 1.0f"):
        assert all(GD.same_bits(a, b) for a, b in zip(runs[form], runs["ftx_adam_step"])), form
    assert not GD.same_bits(runs["ftx_adam_step"][0], torch.from_numpy(base[0]))


# ---------------------------------------------------------------------------------------------------------------- the rules
def own_run(name, base, grads):
    from fusiontransformer_amd import optim
    rule, kwargs, clipped = S.CONFIGS[name]
    max_norm = S.max_norm_for(grads) if clipped else None
    params = S.make_params(base, "cuda")
    assert params[S.OFFSET].data_ptr() % 16 == 4
    opt = getattr(optim, rule)(params, lr=S.LR, weight_decay=S.WD, max_grad_norm=max_norm, **kwargs)
    return S.drive(opt, params, grads, S.STATE_KEYS[rule], "cuda"), max_norm, opt


@pytest.mark.parametrize("name", sorted(S.CONFIGS))
def test_rules_against_float64_at_the_yardsticks_bars(L, data, name):
    base, grads = data
    rule, kwargs, clipped = S.CONFIGS[name]
    shots, max_norm, opt = own_run(name, base, grads)
    assert len(opt._plans) > 0, "the parent's step ran, not the kernel"
    ref = S.reference(rule, kwargs, base, grads, max_norm)
    mine, bar = S.worst(shots, ref), S.yardstick(name, base, grads)
    for k in sorted(bar):
        print("ACC %-22s %-16s kernel %8.3f  torch fp32 on the CPU %8.3f  (units of 2^-24 max|x|)" % (name, k, mine[k], bar[k]))
    assert set(mine) == set(bar)
    for k in bar:
        assert mine[k] <= 2.0 * bar[k], (name, k, mine[k], bar[k])
    if clipped:
        assert 0.25 < float(opt.last_clip_coef) < 0.35 and opt.last_grad_norm.is_cuda and opt.last_grad_norm.dim() == 0
    # cross-check at the bars of test_adam_one_launch_matches_torch_adam: torch's optimizer on the device
    params = S.make_params(base, "cuda", awkward=False)
    topt = getattr(torch.optim, rule)(params, lr=S.LR, weight_decay=S.WD, **kwargs)
    tshots = S.drive(topt, params, grads, S.STATE_KEYS[rule], "cuda", clip=max_norm, awkward=False)
    for a, b in zip(shots, tshots):
        for x, y in zip(a["param"], b["param"]):
            np.testing.assert_allclose(x, y, rtol=2e-6, atol=2e-7)


@pytest.mark.parametrize("rule,kwargs", [("SGD", dict(momentum=0.9, dampening=0.1)), ("AdamW", dict())])
def test_state_dict_moves_both_ways(L, data, rule, kwargs):
    from fusiontransformer_amd import optim
    base, grads = data
    pa, pb = S.make_params(base, "cuda", awkward=False), S.make_params(base, "cuda", awkward=False)
    make = lambda mod, ps: getattr(mod, rule)(ps, lr=S.LR, weight_decay=S.WD, **kwargs)
    oa, ob = make(optim, pa), make(torch.optim, pb)
    keys = S.STATE_KEYS[rule]
    S.drive(oa, pa, grads[:3], keys, "cuda", awkward=False)
    S.drive(ob, pb, grads[:3], keys, "cuda", awkward=False)
    oc, od = make(torch.optim, pa), make(optim, pb)
    oc.load_state_dict(oa.state_dict())                    # our state continues in torch's optimizer ...
    od.load_state_dict(ob.state_dict())                    # ... and torch's in ours (a loaded momentum_buffer is not a first step)
    sc = S.drive(oc, pa, grads[3:5], keys, "cuda", awkward=False)
    sd = S.drive(od, pb, grads[3:5], keys, "cuda", awkward=False)
    assert len(od._plans) > 0
    ref = S.reference(rule, kwargs, base, grads[:5])[-1]
    for x, y, r in zip(sc[-1]["param"], sd[-1]["param"], ref["param"]):
        np.testing.assert_allclose(x, y, rtol=2e-6, atol=2e-7)
        np.testing.assert_allclose(y, r, rtol=2e-6, atol=2e-7)


# ---------------------------------------------------------------------------------------------------------------- the package
class _TwoLayers(torch.nn.Module):
    def __init__(self, w1, w2):
        super().__init__()
        self.a = torch.nn.Parameter(torch.from_numpy(w1.copy()))
        self.b = torch.nn.Parameter(torch.from_numpy(w2.copy()))

    def forward(self, batch):
        return {"lidar_seg_logit": torch.tanh(batch["x"] @ self.a) @ self.b}


def test_train_step_clips_and_schedules_without_a_host_sync(L):
    from fusiontransformer_amd import config, optim
    from fusiontransformer_amd.trainer import TrainStep, build_optimizer, build_scheduler
    rng = np.random.default_rng(4)
    w1, w2 = rng.standard_normal((12, 16)).astype(np.float32), rng.standard_normal((16, 20)).astype(np.float32)
    x = rng.standard_normal((3, 64, 12)).astype(np.float32) * 3
    labels = rng.integers(1, 20, (3, 64))
    cfg = config.lidar_cfg()
    cfg.OPTIMIZER.merge_from_dict({"TYPE": "SGD", "native": True, "MAX_GRAD_NORM": 1.0, "BASE_LR": 0.05, "SGD": {"momentum": 0.9}})
    cfg.SCHEDULER.merge_from_dict({"TYPE": "MultiStepLR", "MultiStepLR": {"milestones": (1,), "gamma": 0.1}})
    model = _TwoLayers(w1, w2).cuda()
    opt = build_optimizer(cfg, model)
    assert type(opt) is optim.SGD and opt.max_grad_norm == 1.0
    step = TrainStep(cfg, model, optimizer=opt, scheduler=build_scheduler(cfg, opt))
    step.fused_loss = False                                # the loss is torch's: only the solver is under test
    ref = R.SGD([w1, w2], 0.05, momentum=0.9, weight_decay=cfg.OPTIMIZER.WEIGHT_DECAY, max_norm=1.0)
    real_step, grads_seen, norms = opt.step, [], []

    def batch(i):
        return {"x": torch.from_numpy(x[i]).cuda(), "seg_label": torch.from_numpy(labels[i]).cuda()}
    step(batch(0))                                         # the warm-up: plans, pinned tables and the norm buffers are made here
    grads_seen.append([model.a.grad.cpu().numpy().copy(), model.b.grad.cpu().numpy().copy()])
    norms.append(float(opt.last_grad_norm))

    def no_sync_step(*a, **k):
        torch.cuda.set_sync_debug_mode("error")
        try:
            return real_step(*a, **k)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    step.optimizer.step = no_sync_step
    step(batch(1))                                         # the momentum buffers exist now: not a first step
    grads_seen.append([model.a.grad.cpu().numpy().copy(), model.b.grad.cpu().numpy().copy()])
    norms.append(float(opt.last_grad_norm))
    assert opt.last_grad_norm.is_cuda and opt.last_clip_coef.is_cuda and opt.last_grad_norm.dim() == 0
    assert len(opt._plans) == 1
    for g, lr, n in zip(grads_seen, (0.05, 0.005), norms):            # p.grad is left unscaled: the reference clips them itself
        ref.step(g, lr)
        assert abs(n - ref.norm) <= 2.0 ** -23 * ref.norm and ref.coef < 1.0
    assert abs(opt.param_groups[0]["lr"] - 0.005) < 1e-12
    for p, r in zip((model.a, model.b), ref.p):
        np.testing.assert_allclose(p.detach().cpu().numpy(), r, rtol=2e-6, atol=2e-7)
