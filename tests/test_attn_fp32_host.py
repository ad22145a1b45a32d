"""The bars of tests/attn_ref.py without a GPU: a numpy fp32 model of the attention kernels' arithmetic stays inside them, and each
defect they exist for, planted into that model, is thrown out.  The GPU tests (tests/test_attn_fp32_gpu.py) hold the real kernels to
the same bars.

One zero key let through the mask only adds exp(-lse) to the row sum (its K and V rows are zero): it is the quiet queries of
attn_ref.make_inputs, with lse near ln T, that show it on the "peaked" inputs, whose other rows have lse >= 13."""
import functools

import pytest

from tests import attn_ref as R

SCALE = 0.125


@functools.lru_cache(maxsize=None)
def case(kind, T):
    return R.Case(kind, 2, T, 2, SCALE)


@pytest.mark.parametrize("T", [1, 2, 31, 33, 70, 129, 257, 578])
@pytest.mark.parametrize("kind", ["gauss", "peaked", "large"])
def test_emulated_kernels_stay_inside_the_bars(kind, T):
    c = case(kind, T)
    for split in (1, 8):
        r, E = c.ratios(R.emulate(c.qkv, c.go, SCALE, split))
        print(R.format_row(f"emulated {kind} T={T} split={split} max|lse|={c.max_lse:.0f}", c.E32, E, r))
        assert R.worst(r) <= 1.0, (kind, T, split, r)


@pytest.mark.parametrize("T", [70, 257])
@pytest.mark.parametrize("kind", ["gauss", "peaked"])
@pytest.mark.parametrize("fault", R.FAULTS)
def test_bars_reject_planted_faults(fault, kind, T):
    """Each fault must exceed the bar on at least one tensor.  Without the fault (fault=None) every one of these cases fails: the
    unplanted model is inside the bars (the test above)."""
    c = case(kind, T)
    r, E = c.ratios(R.emulate(c.qkv, c.go, SCALE, 1, fault=fault))
    print(f"{fault} {kind} T={T}: " + " ".join(f"{n} {max(v):.3g}" for n, v in r.items()))
    assert R.worst(r) > 1.0, (fault, kind, T, r)


def test_bar_is_built_from_the_yardstick_and_the_rounding_counts():
    E32 = {n: (1e-7, 3e-7) for n in R.TENSORS}
    b = R.bar(E32, 40.0)
    assert b["dv"] == (4 * 1e-7 + 4 * R.U * 40.0, 4 * 3e-7 + 4 * R.U * 40.0) and b["out"] == b["dq"] == b["dk"] == b["dv"]
    assert b["lse"] == (4 * 1e-7 + 8 * R.U, 4 * 3e-7 + 8 * R.U)
    assert R.bar(E32, 0.25)["out"] == (4 * 1e-7 + 4 * R.U, 4 * 3e-7 + 4 * R.U)      # max(1, |lse|)
    zero = R.bar({n: (0.0, 0.0) for n in R.TENSORS}, 0.0)
    assert all(v > 0 for pair in zero.values() for v in pair)                       # T = 1: the yardstick is exact


def test_constructed_inputs_do_what_they_are_for():
    """ascending: every key tile raises every query's running maximum.  late_max: every query's largest score is the last token's."""
    import numpy as np
    for T in (70, 257):
        qkv, _ = R.make_inputs("ascending", 2, T, 3)
        s = np.einsum("bqhd,bkhd->bhqk", qkv[:, :, 0].astype(np.float64), qkv[:, :, 1].astype(np.float64))
        tile_max = np.stack([s[..., t0:t0 + 32].max(-1) for t0 in range(0, T, 32)], -1)
        assert (np.diff(tile_max, axis=-1) > 0).all()
        qkv, _ = R.make_inputs("late_max", 2, T, 3)
        s = np.einsum("bqhd,bkhd->bhqk", qkv[:, :, 0].astype(np.float64), qkv[:, :, 1].astype(np.float64))
        assert (s.argmax(-1) == T - 1).all()
