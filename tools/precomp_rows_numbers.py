#!/usr/bin/env python3
"""Many multiscalar muls over one precomputed point set (c25519_precomp_msm_vartime_rows_dev) against the two things a caller could do before
it, on one box in one process (run on the GPU box): m rows of w scalars over the first w of 4096 static points, CompressedEdwardsY out.
    lane / wave   the rows call with the route forced (C25519_PRECOMP_ROWS_LANE / _WAVE), scalars device-resident
    per row       one c25519_precomp_msm_vartime per row (host pointers: the call has no other form; timed on PER_ROW_SAMPLE rows one after
                  the other, as a caller would issue them, the median row scaled to m: every call synchronises, so they do not overlap)
    segments      c25519_msm_vartime_segments_dev with the RAW160 generators replicated into every row, device-resident
Shapes: m = 2^6 .. 2^20 (every power of two for w <= 16, where the two routes cross; every second one for wider rows, and the acceptance
shapes), w in 1, 2, 4, 8, 16, 64, 128, 512, 2048, m x w <= 2^22.  Each figure is the median of REPS calls after a warm-up call of the same
shape, timed with events on the stream (per row: the host clock); min .. max beside it.  The outputs of the two routes are compared byte for
byte at every shape, and with the segments call's.  The acceptance shapes (m = 4096, w = 128; m = 2^17, w = 2; m = 64, w = 2048) are timed
three times over: the larger spread of the two sides' three medians is what a margin has to exceed.  Last, the one-off build of the comb table for handles of
128, 1024 and 4096 points: the first rows call on a fresh handle (one row, one term) against the second.
    python tools/precomp_rows_numbers.py [--out FILE] [--quick]
(writes profiles/precomp_rows_numbers.txt, or FILE, and prints it as it goes)"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "precomp_rows_numbers.txt"))
ap.add_argument("--quick", action="store_true", help="a few shapes only (to try the script)")
args = ap.parse_args()
sys.path.insert(0, ROOT)
import numpy as np
import torch

import curve25519_dalek_amd as pkg

RAW, ED = 2, 0
E = pkg.engine
LANE, WAVE, AUTO = E.PRECOMP_ROWS_LANE, E.PRECOMP_ROWS_WAVE, E.PRECOMP_ROWS_AUTO
REPS = 21
PER_ROW_SAMPLE = 21
N_STATIC = 4096
MAX_TERMS = 1 << 22
ACCEPT = [(4096, 128), (1 << 17, 2), (64, 2048)]
e = pkg.Engine(0)
g = torch.Generator(device="cuda"); g.manual_seed(13)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
fh = open(args.out, "w")


def out(s):
    print(s); sys.stdout.flush()
    fh.write(s + "\n"); fh.flush()


def timed(f, reps=REPS):
    """-> (median, min, max) ms over reps calls of f, events on the stream, after one warm-up call"""
    f()
    ts = []
    for _ in range(reps):
        t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
        t0.record(); f(); t1.record(); t1.synchronize()
        ts.append(t0.elapsed_time(t1))
    return statistics.median(ts), min(ts), max(ts)


def fmt(t):
    return "%9.3f (%8.3f .. %9.3f)" % t


static = e.mul_base_batch(np.random.default_rng(1).integers(0, 256, (N_STATIC, 32), dtype=np.uint8) & np.uint8(0x0F), RAW)
static_dev = torch.from_numpy(static).cuda()
handle = e.precomp_create(static, in_fmt=RAW)
e32, e160 = np.zeros((0, 32), np.uint8), np.zeros((0, 160), np.uint8)


def scalars(m, w):
    s = torch.randint(0, 256, (m, w, 32), device="cuda", generator=g, dtype=torch.uint8)
    s[:, :, 31] &= 0x0F
    return s.contiguous()


def per_row(s_host, w):
    """-> (median, min, max) ms of ONE precomp_msm_vartime over the sample's rows, host clock"""
    ts = []
    e.precomp_msm_vartime(handle, s_host[0], e32, e160, in_fmt=RAW)
    for r in range(s_host.shape[0]):
        t0 = time.perf_counter()
        e.precomp_msm_vartime(handle, s_host[r], e32, e160, in_fmt=RAW)
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def shape(m, w, repeats=1):
    """one line per repeat: lane, wave, per row (scaled to m), segments; -> the figures of every repeat"""
    s = scalars(m, w)
    s_host = s[:PER_ROW_SAMPLE].cpu().numpy()
    flat = s.reshape(m * w, 32)
    pts = static_dev[:w].repeat(m, 1).contiguous()
    off = (np.arange(m + 1, dtype=np.uint64) * np.uint64(w))
    res, rows = {}, []
    for _ in range(repeats):
        lane = timed(lambda: res.__setitem__("lane", e.precomp_msm_vartime_rows_t(handle, s, LANE, ED)))
        wave = timed(lambda: res.__setitem__("wave", e.precomp_msm_vartime_rows_t(handle, s, WAVE, ED)))
        seg = timed(lambda: res.__setitem__("seg", e.msm_vartime_segments_t(flat, pts, off, RAW, ED)))
        one = per_row(s_host, w)
        one = tuple(x * m for x in one)
        assert torch.equal(res["lane"], res["wave"]), "the two routes disagree at m %d w %d" % (m, w)
        assert res["seg"][0] == 0 and torch.equal(res["seg"][1], res["wave"]), "the rows call and the segments call disagree at m %d w %d" % (m, w)
        auto = "lane" if e.precomp_msm_vartime_rows_plan(m, w)[0] == LANE else "wave"
        out("m %8d w %5d | lane %s | wave %s | per row x m %s | segments %s | faster route: %s (AUTO: %s)"
            % (m, w, fmt(lane), fmt(wave), "%11.3f (%10.3f .. %11.3f)" % one, fmt(seg), "lane" if lane[0] < wave[0] else "wave", auto))
        rows.append({"lane": lane, "wave": wave, "per_row": one, "seg": seg, "auto": auto})
    return rows


out("multiplier probe (Engine.microbench(0, 4000), best of 100): %.1f Top/s" % (max(e.microbench(0, 4000) for _ in range(100)) / 1e3))
out("precomp_msm_vartime_rows over %d static points, ms per call: median (min .. max) of %d calls; LANE_WIDTH %d, LANE_MIN_ROWS %d; per row: the median of %d "
    "single calls times m" % (N_STATIC, REPS, E.PRECOMP_ROWS_LANE_WIDTH, E.PRECOMP_ROWS_LANE_MIN_ROWS, PER_ROW_SAMPLE))
t = timed(lambda: e.precomp_msm_vartime_rows_t(handle, scalars(1, 1), WAVE, ED), reps=3)      # (builds the table of the shared handle)
widths = (2, 128) if args.quick else (1, 2, 4, 8, 16, 64, 128, 512, 2048)
for w in widths:
    step = 1 if w <= 16 else 2
    ms = [1 << k for k in range(6, 21, step)]
    if args.quick:
        ms = [64, 4096]
    ms = sorted({m for m in ms + [m for m, ww in ACCEPT if ww == w] + ([4096] if w >= 64 else []) if m * w <= MAX_TERMS})
    for m in ms:
        shape(m, w)
out("-- the acceptance shapes, three times over: AUTO's route against both alternatives; the margin against the spread of the three medians")
for m, w in ([ACCEPT[0]] if args.quick else ACCEPT):
    rows = shape(m, w, repeats=3)
    auto = rows[0]["auto"]
    med = {k: [r[k][0] for r in rows] for k in ("per_row", "seg")}
    med["auto"] = [r[auto][0] for r in rows]
    for k, name in (("per_row", "one precomp_msm_vartime per row"), ("seg", "the replicated segments call")):
        margin = min(med[k]) - max(med["auto"])
        spread = max(max(med[k]) - min(med[k]), max(med["auto"]) - min(med["auto"]))
        out("   m %d w %d: AUTO (%s) %.3f .. %.3f ms, %s %.3f .. %.3f ms: margin %.3f ms, spread of the medians %.3f ms -> %s"
            % (m, w, auto, min(med["auto"]), max(med["auto"]), name, min(med[k]), max(med[k]), margin, spread,
               "AUTO faster x%.2f" % (statistics.median(med[k]) / statistics.median(med["auto"])) if margin > spread else "NOT FASTER beyond the spread"))
out("-- the one-off table build: the first rows call on a fresh handle (one row, one term) against the second, %d handles each" % REPS)
one = scalars(1, 1)
for n in ((128,) if args.quick else (128, 1024, 4096)):
    first, second = [], []
    for _ in range(REPS):
        h = e.precomp_create(static[:n], in_fmt=RAW)
        for dst in (first, second):
            t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
            t0.record(); e.precomp_msm_vartime_rows_t(h, one, WAVE, ED); t1.record(); t1.synchronize()
            dst.append(t0.elapsed_time(t1))
        assert e.precomp_rows_table_bytes(h) == n * 65536
        e.precomp_destroy(h)
    out("   n %5d: first call %8.3f ms (%.3f .. %.3f), second %7.3f ms, table %d MB"
        % (n, statistics.median(first), min(first), max(first), statistics.median(second), n * 65536 >> 20))
e.precomp_destroy(handle)
fh.close()
