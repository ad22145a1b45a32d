"""profiles/attn_fp32_accuracy.txt from the output of `pytest -m gpu tests/test_attn_fp32_gpu.py -s`: every accuracy case as printed on
the GPU, and beside it the same figures of the numpy fp32 model of the kernels (tests/attn_ref.emulate) with the tiling's key groups.

    python tools/attn_accuracy_table.py PYTEST_LOG > profiles/attn_fp32_accuracy.txt
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import attn_ref as R   # noqa: E402

B, H = 2, 3   # tests/test_attn_fp32_gpu.py


def splits(tiling, T):
    """(forward, backward) key groups of a tiling; (0, 0) as attn_config chooses for (B, T, H)."""
    if tiling != (0, 0):
        return tiling[1], tiling[1]
    wave_tiles = -(-T // 32) * H * B
    return (8, 4) if wave_tiles <= 256 else (4, 4) if wave_tiles <= 512 else (2, 2)


def main(log):
    print("# fp32 attention against float64: per tensor  E32 (the float32 yardstick's error)  E (the measured error)  E / bar,")
    print("# max-abs over max-abs (normalisation and bar: tests/attn_ref.py); B = 2, H = 3.  'mi355x' lines as printed by")
    print("# tests/test_attn_fp32_gpu.py on an MI355X, 'emulated' lines from tests/attn_ref.emulate with the same key groups;")
    print("# '>2x: ...' names the tensors whose error on the MI355X is more than twice (or less than half) the emulation's.")
    cases, emu = {}, {}
    for line in open(log):
        m = re.match(r"\.?(acc (\w+) T=(\d+) scale=([\d.]+) tiling=\((\d), (\d)\).*)", line)
        if not m:
            continue
        kind, T, scale, tiling = m.group(2), int(m.group(3)), float(m.group(4)), (int(m.group(5)), int(m.group(6)))
        key = (kind, T, scale)
        if key not in cases:
            cases[key] = R.Case(kind, B, T, H, scale)
        c, sp = cases[key], splits(tiling, T)
        if key + sp not in emu:
            r, E = c.ratios(R.emulate(c.qkv, c.go, scale, sp[0], bwd_split=sp[1]))
            emu[key + sp] = (R.format_row(f"emulated splits={sp} max|lse|={c.max_lse:.0f}", c.E32, E, r), E)
        got = dict((n, float(e)) for n, e in re.findall(r"\| (\w+) \S+ (\S+) \S+", m.group(1)))
        off = [n for n in R.TENSORS if emu[key + sp][1][n][1] > 0 and not 0.5 <= got[n] / emu[key + sp][1][n][1] <= 2.0]
        print("mi355x   " + m.group(1))
        print("         " + emu[key + sp][0] + ("   >2x: " + " ".join(off) if off else ""))


if __name__ == "__main__":
    main(sys.argv[1])
