#!/usr/bin/env python3
"""One shape per row / segment kernel of the Straus family (csrc/straus.h), for comparing two builds of the library on one box (run on the GPU
box): the shapes and the method of seg_msm_numbers.py, precomp_rows_numbers.py and precomp_mixed_numbers.py -- device-resident inputs, RAW160
points in, CompressedEdwardsY out, the median of REPS calls after a warm-up call, timed with events on the stream -- without their other
routes, so that a run takes seconds and two builds can be alternated:
    segments lane   16384 segments x 16 terms          k_mid_seg_straus  (and k_mid_straus_tables, as in every shape with dynamic terms)
    segments wave   1024 segments x 256 terms          k_mid_seg_wave
    rows lane       131072 rows x 2 scalars            k_mid_rows_lane
    rows wave       4096 rows x 128 scalars            k_mid_rows_wave
    mixed lane      131072 rows x (2 + 1), LANE forced k_mid_mixed_lane
    mixed wave      4096 rows x (130 + 17), WAVE forced k_mid_mixed_wave
One process times one build (C25519_HIP_LIB of this tool's environment names another one: tools/devlib.py) and appends one block to FILE:
    C25519_HIP_LIB=/other/libc25519hip.so python tools/straus_family_numbers.py --label parent --out FILE
    python tools/straus_family_numbers.py --label branch --out FILE              (... alternating, at least three times each)
    python tools/straus_family_numbers.py --table FILE                           (the medians side by side, the spread and the verdict per shape)
A shape's spread is max - min of the FIRST label's medians across its blocks; the other label is LEVEL when its median of medians lies within
that spread of the first one's."""
import argparse
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--label", default="this tree")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "straus_family_numbers.txt"))
ap.add_argument("--table", metavar="FILE", help="no GPU: print the side-by-side table of the blocks in FILE")
args = ap.parse_args()

if args.table:
    runs, order = {}, []                                     # shape -> label -> [medians]
    for line in open(args.table):
        m = re.match(r"^\[(.+?)\] (.+?) +\| +([\d.]+) \(", line)
        if m:
            label, shape, med = m.group(1), m.group(2).strip(), float(m.group(3))
            runs.setdefault(shape, {}).setdefault(label, []).append(med)
            if label not in order:
                order.append(label)
    first, other = order[0], order[1]
    print("ms per call, the median of each block; spread = max - min of the %s medians" % first)
    for shape, by in runs.items():
        a, b = by[first], by[other]
        spread = max(a) - min(a)
        ma, mb = statistics.median(a), statistics.median(b)
        verdict = "LEVEL within the spread" if abs(mb - ma) <= spread else ("%s faster x%.3f" % (other, ma / mb) if mb < ma else "%s SLOWER x%.3f" % (other, mb / ma))
        print("%-44s | %s %s -> %.3f | %s %s -> %.3f | spread %.3f (%.1f %%) | %s"
              % (shape, first, " ".join("%.3f" % x for x in a), ma, other, " ".join("%.3f" % x for x in b), mb, spread, 100 * spread / ma, verdict))
    sys.exit(0)

sys.path.insert(0, ROOT)
import numpy as np
import torch

import curve25519_dalek_amd as pkg
import devlib; devlib.apply(pkg)      # (C25519_HIP_LIB of this TOOL's environment selects another build; the package reads no environment)

RAW, ED = 2, 0
E = pkg.engine
LANE, WAVE = E.PRECOMP_ROWS_LANE, E.PRECOMP_ROWS_WAVE
REPS, N_STATIC, POOL = 11, 2050, 4096
e = pkg.Engine(0)
g = torch.Generator(device="cuda"); g.manual_seed(17)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
fh = open(args.out, "a")


def timed(f):
    """-> (median, min, max) ms over REPS calls of f, events on the stream, after one warm-up call"""
    ts = []
    for k in range(REPS + 1):
        t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
        t0.record(); f(); t1.record(); t1.synchronize()
        if k:
            ts.append(t0.elapsed_time(t1))
    return statistics.median(ts), min(ts), max(ts)


def scalars(*shape):
    s = torch.randint(0, 256, shape + (32,), device="cuda", generator=g, dtype=torch.uint8)
    s[..., 31] &= 0x0F
    return s.contiguous()


def terms(n):
    return scalars(n), pool_dev[torch.randint(0, POOL, (n,), device="cuda", generator=g)].contiguous()


def report(shape, f, check):
    res = {}
    t = timed(lambda: res.__setitem__("r", f()))
    assert check(res["r"]), shape
    line = "[%s] %-44s | %9.3f (%8.3f .. %9.3f)" % ((args.label, shape) + t)
    print(line); sys.stdout.flush()
    fh.write(line + "\n"); fh.flush()


rng = np.random.default_rng(1)
pool = e.mul_base_batch(rng.integers(0, 256, (POOL, 32), dtype=np.uint8) & np.uint8(0x0F), RAW)
pool_dev = torch.from_numpy(pool).cuda()
handle = e.precomp_create(pool[:N_STATIC], in_fmt=RAW)
e.precomp_msm_vartime_rows_t(handle, scalars(1, 1), WAVE, ED)       # (builds the comb table of the handle)
seg_ok = lambda r: r[0] == 0 and bool(r[2].all())
for m, k in ((16384, 16), (1024, 256)):
    assert E.MSM_SEGMENT_DIRECT_MAX < 256 <= E.MSM_SEGMENT_WAVE_MAX and m * k <= E.MSM_SEGMENT_PASS_TERMS
    s, p = terms(m * k)
    off = np.arange(m + 1, dtype=np.uint64) * np.uint64(k)
    plan = e.msm_vartime_segments_plan(off)
    assert plan[:4] == ((m, 0, 0, 1) if k <= E.MSM_SEGMENT_DIRECT_MAX else (0, m, 0, 1)), plan
    report("segments %s %d x %d" % ("lane" if plan[0] else "wave", m, k), lambda: e.msm_vartime_segments_t(s, p, off, RAW, ED), seg_ok)
for m, w, route in ((1 << 17, 2, LANE), (4096, 128, WAVE)):
    ss = scalars(m, w)
    report("rows %s %d x %d" % ("lane" if route == LANE else "wave", m, w), lambda: e.precomp_msm_vartime_rows_t(handle, ss, route, ED), lambda r: r.shape == (m, 32))
for m, w, k, route in ((1 << 17, 2, 1, LANE), (4096, 130, 17, WAVE)):
    ss = scalars(m, w)
    s, p = terms(m * k)
    off = np.arange(m + 1, dtype=np.uint64) * np.uint64(k)
    report("mixed %s %d x (%d + %d)" % ("lane" if route == LANE else "wave", m, w, k),
           lambda: e.precomp_msm_vartime_mixed_rows_t(handle, ss, s, p, off, RAW, route, ED), seg_ok)
e.precomp_destroy(handle)
fh.close()
