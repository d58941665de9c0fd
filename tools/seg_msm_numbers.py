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
    python tools/seg_msm_numbers.py   (writes profiles/seg_msm_numbers.txt and prints it)"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import curve25519_dalek_amd as pkg

RAW, ED = 2, 0
REPS = 7
A_SAMPLE = 2048
e = pkg.Engine(0)
ev = pkg.Engine(0, flags=pkg.engine.FLAG_VARTIME_TABLES)
L, T = pkg.engine.MSM_SEGMENT_DIRECT_MAX, pkg.engine.MSM_SEGMENT_PASS_TERMS
g = torch.Generator(device="cuda"); g.manual_seed(11)
lines = []


def out(s):
    print(s); sys.stdout.flush()
    lines.append(s)


def warm():
    for _ in range(40):
        e.microbench(0, 4000)


def timed(f):
    """-> (median, min, max) ms over REPS runs of f, events on the stream, after one warm-up run"""
    warm(); f()
    ts = []
    for _ in range(REPS):
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


def route_a(s, pts, off, count):
    lib, ctx = e.lib, e.ctx
    buf = np.zeros(32, np.uint8)
    sp, pp, bp = s.data_ptr(), pts.data_ptr(), buf.ctypes.data
    e._bind_stream()
    for k in range(count):
        a, b = int(off[k]), int(off[k + 1])
        st = lib.c25519_msm_vartime_dev(ctx, sp + 32 * a, pp + 160 * a, b - a, RAW, ED, bp)
        assert st == 0, st


def fmt(t):
    return "%9.3f (%8.3f .. %8.3f)" % t


def verdict(new, other):
    """who wins, or a tie when the difference is within the repeats' spreads"""
    spread = max(new[2] - new[1], other[2] - other[1])
    if abs(new[0] - other[0]) <= spread:
        return "tie"
    return "new x%.1f" % (other[0] / new[0]) if new[0] < other[0] else "NEW LOSES x%.1f" % (new[0] / other[0])


def case(name, lengths, with_a=True, with_b=True):
    lengths = np.asarray(lengths, dtype=np.int64)
    m, n = len(lengths), int(lengths.sum())
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    off_dev = torch.from_numpy(off.astype(np.int64)).cuda()
    s, pts = inputs(n)
    res = {}
    new = timed(lambda: res.__setitem__("new", e.msm_vartime_segments_t(s, pts, off, RAW, ED)))
    assert res["new"][0] == 0
    row = "%-26s m %7d n %8d | new %s" % (name, m, n, fmt(new))
    if with_a:
        cnt = min(m, A_SAMPLE)
        a = timed(lambda: route_a(s, pts, off, cnt))
        a = tuple(x * m / cnt for x in a)
        row += " | A %s %-16s" % (fmt(a), verdict(new, a))
    if with_b:
        def fb():
            prod, _ = ev.mul_batch_t(s, pts, RAW, RAW)
            res["b"] = ev.point_sum_segments_t(prod, off_dev, RAW, ED)
        b = timed(fb)
        assert torch.equal(res["new"][1], res["b"][1]), "the new call and route B disagree at %s" % name
        row += " | B %s %-16s" % (fmt(b), verdict(new, b))
    out(row)
    return new


out("segmented vartime MSM, ms per call: median (min .. max) of %d repeats; DIRECT_MAX %d, PASS_TERMS %d; route A scaled from its first %d segments" % (REPS, L, T, A_SAMPLE))
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
out("-- passes: 2^20 terms are four passes of C25519_MSM_SEGMENT_PASS_TERMS; per term they should cost what one pass costs")
one = case("len 4, 2^18 terms", [4] * (N // 4), with_a=False, with_b=False)
four = case("len 4, 2^20 terms", [4] * N, with_a=False, with_b=False)
out("   ns per term: one pass %.2f, four passes %.2f" % (one[0] * 1e6 / N, four[0] * 1e6 / (4 * N)))
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "seg_msm_numbers.txt"), "w") as fh:
    fh.write("\n".join(lines) + "\n")
