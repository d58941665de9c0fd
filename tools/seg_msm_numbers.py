#!/usr/bin/env python3
"""The segmented vartime MSM (c25519_msm_vartime_segments_dev) against the two routes a caller had before it, on one box in one run
(run on the GPU box): device-resident RAW160 points, CompressedEdwardsY sums out, m segments of `len` terms with m x len = 2^18 for
len 2, 4, 16, 64, and one mix of random lengths 0 .. 64.
    new      one c25519_msm_vartime_segments_dev call
    route A  one c25519_msm_vartime_dev call per segment (timed on the first 2048 segments, one after the other as a caller would issue
             them, and scaled to m: every call synchronises, so the calls do not overlap)
    route B  c25519_mul_batch_dev on a FLAG_VARTIME_TABLES context, then c25519_point_sum_segments_dev
Each figure is the median of 7 repeats after a warm-up run of the same shape, timed with events on the stream; the spread (min .. max) is
printed beside it, and a difference smaller than the spreads is reported as a tie.  The outputs of the new call and of route B are
compared byte for byte at every timed shape.  Two more rows per constant of the header: segments just below and just above
C25519_MSM_SEGMENT_DIRECT_MAX (the per-lane chain against one single-MSM call per segment), and 2^20 terms (four passes of
C25519_MSM_SEGMENT_PASS_TERMS) beside the 2^18 terms of one pass.
The wave route (more than DIRECT_MAX and at most C25519_MSM_SEGMENT_WAVE_MAX terms, one wave per segment): len 65 .. 4096, each at m = 1, 64
and 4096 segments (m capped so that m x len <= 2^20), and the pair just below and just above WAVE_MAX; route A beside every row -- what a
tree without the wave route does for these lengths inside the call, one single-MSM call per segment.  The outputs are compared with route A's
on the first segments.  A tree whose engine has no MSM_SEGMENT_WAVE_MAX (before the wave route) runs the same rows: run the script on
both trees on one box in one session, the second time with --append, to see what the route changed.
The bucket route (more than WAVE_MAX and at most C25519_MSM_SEGMENT_BUCKET_MAX terms, every such segment of a call side by side): segments x
terms of 8 / 64 / 512 x 2049, 64 / 1024 x 4096, 64 x 8192, 64 / 256 x 16384, 64 x 32768, 16 / 64 x 65536, and one lone segment of each length;
median of 5 repeats.  A tree before the bucket route runs the same rows on its single-MSM route: `--section long` runs these rows alone, for
the two runs on one box in one session.
    python tools/seg_msm_numbers.py [--root TREE] [--label TEXT] [--append] [--out FILE] [--section all|long]
(writes profiles/seg_msm_numbers.txt of this tree, or FILE, and prints it; --root: import the package from another checkout, built there)"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=ROOT, help="the checkout whose package and library are timed")
ap.add_argument("--label", default="", help="a line that names the tree in the output")
ap.add_argument("--append", action="store_true", help="append to the output file instead of replacing it")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_msm_numbers.txt"))
ap.add_argument("--section", default="all", choices=("all", "long"), help="long: only the rows of the bucket route's lengths")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import numpy as np
import torch

import curve25519_dalek_amd as pkg

RAW, ED = 2, 0
REPS = 7
A_SAMPLE = 2048
e = pkg.Engine(0)
ev = pkg.Engine(0, flags=pkg.engine.FLAG_VARTIME_TABLES)
L, T = pkg.engine.MSM_SEGMENT_DIRECT_MAX, pkg.engine.MSM_SEGMENT_PASS_TERMS
HAS_WAVE = hasattr(pkg.engine, "MSM_SEGMENT_WAVE_MAX")
W = pkg.engine.MSM_SEGMENT_WAVE_MAX if HAS_WAVE else 4096     # a tree before the wave route: the same rows, all on its single-MSM route
g = torch.Generator(device="cuda"); g.manual_seed(11)
lines = []


def out(s):
    print(s); sys.stdout.flush()
    lines.append(s)


def warm():
    for _ in range(40):
        e.microbench(0, 4000)


def timed(f, reps=None):
    """-> (median, min, max) ms over REPS runs of f, events on the stream, after one warm-up run"""
    warm(); f()
    ts = []
    for _ in range(reps or REPS):
        t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
        t0.record(); f(); t1.record(); t1.synchronize()
        ts.append(t0.elapsed_time(t1))
    return statistics.median(ts), min(ts), max(ts)


table = torch.from_numpy(e.mul_base_batch(np.random.default_rng(1).integers(0, 256, (256, 32), dtype=np.uint8) & np.uint8(0x0F), 2)).cuda()


def inputs(n):
    pts = table[torch.randint(0, 256, (n,), device="cuda", generator=g)].contiguous()
    s = torch.randint(0, 256, (n, 32), device="cuda", generator=g, dtype=torch.uint8)
    s[:, 31] &= 0x0F
    return s.contiguous(), pts


def route_a(s, pts, off, count, keep=None):
    lib, ctx = e.lib, e.ctx
    buf = np.zeros(32, np.uint8)
    sp, pp, bp = s.data_ptr(), pts.data_ptr(), buf.ctypes.data
    e._bind_stream()
    for k in range(count):
        a, b = int(off[k]), int(off[k + 1])
        st = lib.c25519_msm_vartime_dev(ctx, sp + 32 * a, pp + 160 * a, b - a, RAW, ED, bp)
        assert st == 0, st
        if keep is not None:
            keep.append(bytes(buf))


def fmt(t):
    return "%9.3f (%8.3f .. %8.3f)" % t


def verdict(new, other):
    """who wins, or a tie when the difference is within the repeats' spreads"""
    spread = max(new[2] - new[1], other[2] - other[1])
    if abs(new[0] - other[0]) <= spread:
        return "tie"
    return "new x%.1f" % (other[0] / new[0]) if new[0] < other[0] else "NEW LOSES x%.1f" % (new[0] / other[0])


def case(name, lengths, with_a=True, with_b=True, check_a=0, reps=None):
    lengths = np.asarray(lengths, dtype=np.int64)
    m, n = len(lengths), int(lengths.sum())
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    off_dev = torch.from_numpy(off.astype(np.int64)).cuda()
    s, pts = inputs(n)
    res = {}
    new = timed(lambda: res.__setitem__("new", e.msm_vartime_segments_t(s, pts, off, RAW, ED)), reps)
    assert res["new"][0] == 0
    row = "%-26s m %7d n %8d | new %s" % (name, m, n, fmt(new))
    if with_a:
        cnt = min(m, A_SAMPLE)
        a = timed(lambda: route_a(s, pts, off, cnt), reps)
        a = tuple(x * m / cnt for x in a)
        row += " | A %s %-16s" % (fmt(a), verdict(new, a))
    if check_a:                                              # the first check_a sums against the single call's, byte for byte (also without route A's timing)
        keep = []
        route_a(s, pts, off, min(m, check_a), keep)
        got = res["new"][1][:len(keep)].cpu().numpy()
        assert [bytes(got[k]) for k in range(len(keep))] == keep, "the new call and route A disagree at %s" % name
    if with_b:
        def fb():
            prod, _ = ev.mul_batch_t(s, pts, RAW, RAW)
            res["b"] = ev.point_sum_segments_t(prod, off_dev, RAW, ED)
        b = timed(fb)
        assert torch.equal(res["new"][1], res["b"][1]), "the new call and route B disagree at %s" % name
        row += " | B %s %-16s" % (fmt(b), verdict(new, b))
    out(row)
    return new


if args.label:
    out("==== " + args.label)
out("multiplier probe (Engine.microbench(0, 4000), best of 100): %.1f Top/s" % (max(e.microbench(0, 4000) for _ in range(100)) / 1e3))
out("segmented vartime MSM, ms per call: median (min .. max) of %d repeats; DIRECT_MAX %d, WAVE_MAX %s, PASS_TERMS %d; route A scaled from its first %d segments"
    % (REPS, L, W if HAS_WAVE else "none (no wave route in this tree)", T, A_SAMPLE))


def long_section():
    bmax = getattr(pkg.engine, "MSM_SEGMENT_BUCKET_MAX", None)
    out("-- the bucket route: more than WAVE_MAX and at most BUCKET_MAX (%s) terms; median of 5 repeats; route A where m <= 64"
        % (bmax if bmax else "none: no bucket route in this tree, every row is one single-MSM call per segment inside the call"))
    for m, ln in ((8, 2049), (64, 2049), (512, 2049), (64, 4096), (1024, 4096), (64, 8192), (64, 16384), (256, 16384), (64, 32768), (16, 65536), (64, 65536)):
        case("%d x %d" % (m, ln), [ln] * m, with_a=m <= 64, with_b=False, check_a=2, reps=5)
    for ln in (2049, 4096, 16384, 65536):
        case("1 x %d" % ln, [ln], with_b=False, check_a=1, reps=5)


if args.section == "long":
    long_section()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as fh:
        fh.write("\n".join(lines) + "\n")
    sys.exit(0)
N = 1 << 18
for ln in (2, 4, 16, 64):
    case("len %d" % ln, [ln] * (N // ln))
mix = np.random.default_rng(3).integers(0, 65, size=N // 32)
case("mix of lengths 0 .. 64", mix)
case("mix, sorted by length", np.sort(mix))
out("-- around C25519_MSM_SEGMENT_DIRECT_MAX: the per-lane chain against one single-MSM call per segment")
for m in (64, 1024):
    case("len %d (direct)" % L, [L] * m, with_b=False)
    case("len %d (long route)" % (L + 1), [L + 1] * m, with_b=False)
out("-- the wave route: more than DIRECT_MAX and at most WAVE_MAX terms, one wave per segment; m = 1, 64, 4096 capped at m x len <= 2^20")
for ln in (65, 128, 256, 512, 1024, 2048, 4096):
    for m in sorted({min(m, (1 << 20) // ln) for m in (1, 64, 4096)}):
        case("len %d" % ln, [ln] * m, with_b=False, check_a=2)
out("-- around C25519_MSM_SEGMENT_WAVE_MAX: one wave against one single-MSM call per segment")
for m in (64, (1 << 20) // (W + 1)):
    case("len %d (wave)" % W, [W] * m, with_b=False, check_a=2)
    case("len %d (single-MSM route)" % (W + 1), [W + 1] * m, with_b=False, check_a=2)
long_section()
out("-- passes: 2^20 terms are four passes of C25519_MSM_SEGMENT_PASS_TERMS; per term they should cost what one pass costs")
one = case("len 4, 2^18 terms", [4] * (N // 4), with_a=False, with_b=False)
four = case("len 4, 2^20 terms", [4] * N, with_a=False, with_b=False)
out("   ns per term: one pass %.2f, four passes %.2f" % (one[0] * 1e6 / N, four[0] * 1e6 / (4 * N)))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a" if args.append else "w") as fh:
    fh.write("\n".join(lines) + "\n")
