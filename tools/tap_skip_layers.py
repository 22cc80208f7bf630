#!/usr/bin/env python3
"""Per-layer A/B of the pixel-major tiles (rn_ctx_set_tap_skip): tools/layer_report.py --tune with RN_TAP_SKIP=1
(never) and RN_TAP_SKIP=2 (wherever eligible), alternating, each run a fresh process under its own time limit.

    python tools/tap_skip_layers.py [--rounds 3] [--timeout 240] > profiles/tap_skip/layers_off_against_on.txt

Per 3x3 layer: the runs' ms off and on, the medians, the spread of the off runs (largest minus smallest) and
whether the on median is faster by more than that spread -- the rule of mode 0 takes exactly those layers.  The
first run that fails ends the script."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(mode, timeout, extra):
    env = dict(os.environ, RN_TAP_SKIP=str(mode))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "layer_report.py"), "--tune"] + extra, env=env,
                       capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        sys.exit(f"layer_report.py failed with RN_TAP_SKIP={mode} (status {r.returncode})")
    rows, total = [], None
    for line in r.stdout.splitlines():
        f = line.split()
        if line.startswith("total "):
            total = float(f[1])
        elif len(f) >= 6 and f[0].startswith("conv2d"):
            rows.append((f[1], float(f[2])))
    return rows, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240)
    a, extra = ap.parse_known_args()
    off, on, tot = [], [], {1: [], 2: []}
    for _ in range(a.rounds):
        for mode, dst in ((1, off), (2, on)):
            rows, total = run(mode, a.timeout, extra)
            dst.append(rows)
            tot[mode].append(total)
    print(f"tools/layer_report.py --tune {' '.join(extra)}: RN_TAP_SKIP=1 (off) against 2 (on), {a.rounds} alternations; ms")
    print(f"{'layer':24s} {'off runs':>24s} {'on runs':>24s} {'off med':>8s} {'on med':>8s} {'gain':>7s} {'off spread':>10s}  verdict")
    gain_sum = 0.0
    for i, (name, _) in enumerate(off[0]):
        if not name.endswith(".conv2"):
            continue
        o, n = [r[i][1] for r in off], [r[i][1] for r in on]
        mo, mn, spread = statistics.median(o), statistics.median(n), max(o) - min(o)
        verdict = "faster" if mo - mn > spread else ("slower" if mn - mo > spread else "within the spread")
        gain_sum += mo - mn
        print(f"{name:24s} {' '.join(f'{v:7.3f}' for v in o):>24s} {' '.join(f'{v:7.3f}' for v in n):>24s} {mo:8.3f} {mn:8.3f} "
              f"{mo - mn:+7.3f} {spread:10.3f}  {verdict}")
    print(f"sum of the 3x3 layers' gains {gain_sum:+.3f} ms; forward by events: off {' '.join(f'{v:.3f}' for v in tot[1])}, "
          f"on {' '.join(f'{v:.3f}' for v in tot[2])}")


if __name__ == "__main__":
    main()
