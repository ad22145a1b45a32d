"""profiles/attn_fp32_accuracy.txt and profiles/attn_bf16_accuracy.txt from the output of
`pytest -m gpu tests/test_attn_bf16_gpu.py tests/test_attn_fp32_gpu.py -s`: every accuracy case as printed on the GPU, and beside it
the same figures of the numpy model of the kernels (tests/attn_ref.emulate / emulate_bf16) with the tiling's key groups.

    python tools/attn_accuracy_table.py PYTEST_LOG > profiles/attn_fp32_accuracy.txt
    python tools/attn_accuracy_table.py --bf16 PYTEST_LOG > profiles/attn_bf16_accuracy.txt
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import attn_ref as R   # noqa: E402

B, H = 2, 3   # tests/test_attn_fp32_gpu.py, tests/test_attn_bf16_gpu.py


def splits(tiling, T):
    """(forward, backward) key groups of a tiling; (0, 0) as attn_config chooses for (B, T, H)."""
    if tiling != (0, 0):
        return tiling[1], tiling[1]
    wave_tiles = -(-T // 32) * H * B
    return (8, 4) if wave_tiles <= 256 else (4, 4) if wave_tiles <= 512 else (2, 2)


def main(log, bf16):
    if bf16:
        head = ["# bf16-operand attention against float64 on the bf16-rounded operands: per tensor  E_yard (the error of the contract stated",
                "# unfused in float64, attn_ref.yardstick_bf16; for lse: of the float32 reference)  E (the measured error)  E / bar,",
                "# max-abs over max-abs (normalisation and bar: tests/attn_ref.py, bar_bf16); B = 2, H = 3.  'mi355x' lines as printed by",
                "# tests/test_attn_bf16_gpu.py on an MI355X, 'emulated' lines from tests/attn_ref.emulate_bf16 with the same key groups;",
                "# '>2x: ...' names the tensors whose error on the MI355X is more than twice (or less than half) the emulation's."]
        pattern, new_case, emulate, yard = r"\.*bf16 (acc (\w+) T=(\d+) scale=([\d.]+) tiling=\((\d), (\d)\).*)", R.CaseBf16, R.emulate_bf16, "E_bar"
    else:
        head = ["# fp32 attention against float64: per tensor  E32 (the float32 yardstick's error)  E (the measured error)  E / bar,",
                "# max-abs over max-abs (normalisation and bar: tests/attn_ref.py); B = 2, H = 3.  'mi355x' lines as printed by",
                "# tests/test_attn_fp32_gpu.py on an MI355X, 'emulated' lines from tests/attn_ref.emulate with the same key groups;",
                "# '>2x: ...' names the tensors whose error on the MI355X is more than twice (or less than half) the emulation's."]
        pattern, new_case, emulate, yard = r"\.*(acc (\w+) T=(\d+) scale=([\d.]+) tiling=\((\d), (\d)\).*)", R.Case, R.emulate, "E32"
    cases, emu, rows = {}, {}, []
    worst = {n: (0.0, "") for n in R.TENSORS}
    for line in open(log):
        m = re.match(pattern, line)
        if not m:
            continue
        kind, T, scale, tiling = m.group(2), int(m.group(3)), float(m.group(4)), (int(m.group(5)), int(m.group(6)))
        key = (kind, T, scale)
        if key not in cases:
            cases[key] = new_case(kind, B, T, H, scale)
        c, sp = cases[key], splits(tiling, T)
        if key + sp not in emu:
            r, E = c.ratios(emulate(c.qkv, c.go, scale, sp[0], bwd_split=sp[1]))
            emu[key + sp] = (R.format_row(f"emulated splits={sp} max|lse|={c.max_lse:.0f}", getattr(c, yard), E, r), E)
        got = dict((n, float(e)) for n, e in re.findall(r"\| (\w+) \S+ (\S+) \S+", m.group(1)))
        for n, ratio in re.findall(r"\| (\w+) \S+ \S+ (\S+)", m.group(1)):
            if float(ratio) > worst[n][0]:
                worst[n] = (float(ratio), f"{kind} T={T} scale={scale} tiling={tiling}")
        off = [n for n in R.TENSORS if emu[key + sp][1][n][1] > 0 and not 0.5 <= got[n] / emu[key + sp][1][n][1] <= 2.0]
        rows.append("mi355x   " + m.group(1))
        rows.append("         " + emu[key + sp][0] + ("   >2x: " + " ".join(off) if off else ""))
    print("\n".join(head))
    if bf16:
        print(f"# worst E / bar on the MI355X over the {len(rows) // 2} (case, tiling) lines:")
        for n in R.TENSORS:
            print(f"#   {n:3s} {worst[n][0]:.2f}   {worst[n][1]}")
    print("\n".join(rows))


if __name__ == "__main__":
    main(sys.argv[-1], "--bf16" in sys.argv[1:-1])
