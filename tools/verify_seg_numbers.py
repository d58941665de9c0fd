#!/usr/bin/env python3
"""The segmented verify_batch (ed25519_verify_batch_segments_dev) against the two routes a caller with many independent batches had before it, on one
box in one run (run on the GPU box): 2^16 honest signatures over 32-byte messages, device-resident, cut into segments of 1, 4, 16, 64, 256 and 1023
signatures.
    new   one ed25519_verify_batch_segments_dev call
    (a)   one ed25519_verify_batch_keys_dev call per segment, one after the other as a caller would issue them (every call synchronises, so the
          calls do not overlap); timed on the first A_SAMPLE segments and scaled to m
    (b)   one ed25519_verify_each_dev over all 2^16 signatures: per-signature verdicts, no batching
(a) and (b) are code the segmented call does not change.  Device z-mode with the keys' cached points and with key bytes; the transcript z-mode (one
Merlin transcript per segment on the host, one synchronisation in the middle of the call) in rows of its own.  After a warm-up run of every arm the three
arms ALTERNATE, REPS rounds in one process; each figure is the median with (min .. max) beside it, and a difference within the spreads is a tie.  The
statuses of the new call are checked to be all OK at every shape, and with one forged signature per 97 segments against the positions forged.
Then the break-even: the smallest number of segments m (powers of two) from which the new call beats (a), per length; 2^20 signatures in segments
of 4, 64 and 256 (several passes of the segmented MSM); and a proxy for what the call's second synchronisation costs.
    python tools/verify_seg_numbers.py [--out FILE]
(writes profiles/verify_seg_numbers.txt of this tree, or FILE, and prints it)"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_seg_numbers.txt"))
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
sys.path.insert(0, ROOT)
import numpy as np
import torch

import curve25519_dalek_amd as pkg

REPS = args.reps
A_SAMPLE = 512
N = 1 << 16
NBIG = 1 << 20                                              # the last section: the same lengths when the segments fill the GPU
MSG = 32
LENS = (1, 4, 16, 64, 256, 1023)
e = pkg.Engine(0)
lines = []


def out(s):
    print(s); sys.stdout.flush()
    lines.append(s)


def warm():
    for _ in range(20):
        e.microbench(0, 4000)


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ts):
    return statistics.median(ts), min(ts), max(ts)


def fmt(t):
    return "%9.3f (%8.3f .. %8.3f)" % t


def verdict(new, other):
    spread = max(new[2] - new[1], other[2] - other[1])
    if abs(new[0] - other[0]) <= spread:
        return "tie"
    return "new x%.1f" % (other[0] / new[0]) if new[0] < other[0] else "NEW LOSES x%.1f" % (new[0] / other[0])


# honest signatures, made on the GPU (the first 2^16 of them serve every section but the last)
g = torch.Generator(device="cuda"); g.manual_seed(12)
seeds = torch.randint(0, 256, (NBIG, 32), device="cuda", generator=g, dtype=torch.uint8)
msgs = torch.randint(0, 256, (NBIG * MSG,), device="cuda", generator=g, dtype=torch.uint8)
moff = (torch.arange(NBIG + 1, dtype=torch.int64) * MSG).cuda()
pks, sigs = e.sign_batch_t(seeds, msgs, moff)
points = e.decompress_batch_t(pks)
points = (points[1] if isinstance(points, tuple) else points).contiguous()


def offsets(ln, m=None, total=N):
    m = total // ln if m is None else m
    return (np.arange(m + 1, dtype=np.uint64) * ln)


def route_a(off, count, z_mode, pp):
    lib, ctx = e.lib, e.ctx
    e._bind_stream()
    mp, op, sp, kp = msgs.data_ptr(), moff.data_ptr(), sigs.data_ptr(), pks.data_ptr()
    for k in range(count):
        a, b = int(off[k]), int(off[k + 1])
        st = lib.ed25519_verify_batch_keys_dev(ctx, mp, op + 8 * a, NBIG * MSG, sp + 64 * a, kp + 32 * a, (pp.data_ptr() + 160 * a) if pp is not None else None, b - a, z_mode)
        assert st == 0, st


def case(ln, z_mode, pp, m=None, with_b=True, check=True, total=N):
    off = offsets(ln, m, total)
    m = off.shape[0] - 1
    n = int(off[-1])
    cnt = min(m, A_SAMPLE)
    mm, mo, ss, kk = msgs[:n * MSG], moff[:n + 1], sigs[:n], pks[:n]
    ppn = pp[:n] if pp is not None else None
    res = {}
    f_new = lambda: res.__setitem__("new", e.verify_batch_segments_t(mm, mo, ss, kk, off, z_mode, pk_points=ppn))
    f_a = lambda: route_a(off, cnt, z_mode, pp)
    f_b = lambda: res.__setitem__("b", e.verify_each_t(mm, mo, ss, kk))
    warm(); f_new(); f_a()
    if with_b:
        f_b()
    tn, ta, tb = [], [], []
    for _ in range(REPS):
        tn.append(wall(f_new)); ta.append(wall(f_a) * m / cnt)
        if with_b:
            tb.append(wall(f_b))
    assert not bool(res["new"].any()), "an honest segment was rejected"
    if check:                                                # one forged signature in every 97th segment
        bad = list(range(0, m, 97))
        fm = mm.clone()
        for s in bad:
            fm[int(off[s]) * MSG + 3] ^= 1
        got = e.verify_batch_segments_t(fm, mo, ss, kk, off, z_mode, pk_points=ppn).cpu().numpy()
        want = np.zeros(m, np.uint8); want[bad] = 3
        assert np.array_equal(got, want), "forged segments: wrong statuses"
    new, a = stats(tn), stats(ta)
    row = "len %4d m %6d n %7d | new %s | (a) %s %-16s" % (ln, m, n, fmt(new), fmt(a), verdict(new, a))
    if with_b:
        b = stats(tb)
        row += " | (b) %s %-16s" % (fmt(b), verdict(new, b))
    out(row)
    return new, a


out("multiplier probe (Engine.microbench(0, 4000), best of 100): %.1f Top/s" % (max(e.microbench(0, 4000) for _ in range(100)) / 1e3))
out("segmented verify_batch, ms per call, wall clock around the call and a device synchronisation: median (min .. max) of %d alternating rounds; "
    "%d signatures of %d-byte messages; (a) scaled from its first %d segments" % (REPS, N, MSG, A_SAMPLE))
for name, z_mode, pp in (("device z-mode, cached key points", 1, points), ("device z-mode, key bytes", 1, None),
                         ("transcript z-mode, cached key points", 0, points), ("transcript z-mode, key bytes", 0, None)):
    out("-- " + name)
    for ln in LENS:
        case(ln, z_mode, pp)
out("-- break-even against (a), device z-mode, cached key points: m segments of one length (m a power of two), the smallest m from which the new call wins")
for ln in LENS:
    found = None
    for m in (1, 2, 4, 8, 16, 32, 64):
        if m * ln > N:
            break
        new, a = case(ln, 1, points, m=m, with_b=False, check=False)
        if found is None and new[0] < a[0] and verdict(new, a) != "tie":
            found = m
    out("   len %d: the new call wins from m = %s" % (ln, found if found is not None else "more than 64 (or never at this size)"))
out("-- 2^20 signatures, device z-mode, cached key points: more segments than one pass of the segmented MSM holds (C25519_MSM_SEGMENT_PASS_TERMS terms: %d segments of 64, %d of 256)"
    % (pkg.engine.MSM_SEGMENT_PASS_TERMS // 129, pkg.engine.MSM_SEGMENT_PASS_TERMS // 513))
for ln in (4, 64, 256):
    case(ln, 1, points, total=NBIG, check=False)


# what the second synchronisation of the call costs (the segmented MSM synchronises once; the verdict kernel, the 8-byte copy of the hash kernel's
# counters and a second hipStreamSynchronize follow): a proxy -- one tiny kernel, an 8-byte copy to pinned memory and a stream synchronisation
x = torch.zeros(64, device="cuda", dtype=torch.uint8)
h = torch.empty(8, dtype=torch.uint8).pin_memory()
ts = []
for _ in range(200):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    x.add_(1); h.copy_(x[:8], non_blocking=True); torch.cuda.current_stream().synchronize()
    ts.append((time.perf_counter() - t0) * 1e6)
out("-- the second synchronisation (proxy: a tiny kernel, an 8-byte copy to pinned memory, a stream synchronisation), us: median %.1f (min %.1f .. max %.1f) of 200"
    % (statistics.median(ts[20:]), min(ts[20:]), max(ts[20:])))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
