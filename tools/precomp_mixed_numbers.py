#!/usr/bin/env python3
"""Many mixed multiscalar muls over one precomputed point set (c25519_precomp_msm_vartime_mixed_rows_dev) against the two things a caller could
do before it, on one box in one process (run on the GPU box): m rows of w static scalars over the first w of 2050 static points plus k dynamic
terms of their own, RAW160 dynamic points, CompressedEdwardsY out.
    lane / wave    the mixed rows call with the route forced (C25519_PRECOMP_ROWS_LANE / _WAVE), inputs device-resident
    composition    the three calls of INTEGRATION.md section 3.4: c25519_precomp_msm_vartime_rows_dev -> RAW160, c25519_msm_vartime_segments_dev ->
                   RAW160, c25519_point_add_batch_dev -> CompressedEdwardsY, inputs device-resident
    per row        one c25519_precomp_msm_vartime per row (host pointers: the call has no other form; timed on at most PER_ROW_SAMPLE rows one
                   after the other, as a caller would issue them, the median row scaled to m: every call synchronises, so they do not overlap)
Shapes (rows x (static + dynamic)): 4096 x (130 + 17), 256 x (2050 + 40), 131072 x (2 + 1), 2^20 x (1 + 2), 64 x (2048 + 64), and few short
rows: 4096 x (2 + 1).  Each figure is the median of REPS calls (FEW_REPS where one call takes longer than SLOW_MS) after a warm-up call of
the same shape, timed with events on the stream (per row: the host clock); min .. max beside it.  Every shape is timed three times over, the
paths alternating: the larger spread of the two sides' three medians is what a margin has to exceed.  The outputs of the two routes and of
the composition are compared byte for
byte at every shape.  Last, the two routes alone across m = 2^9 .. 2^17 for narrow rows (w < LANE_WIDTH, k <= DIRECT_MAX: the shapes AUTO
chooses between them for), FEW_REPS calls each: where they cross.
    python tools/precomp_mixed_numbers.py [--out FILE] [--quick] [--sweep W,K ...]
(writes profiles/precomp_mixed_numbers.txt, or FILE, and prints it as it goes)"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "precomp_mixed_numbers.txt"))
ap.add_argument("--quick", action="store_true", help="small shapes only (to try the script)")
ap.add_argument("--sweep", nargs="+", metavar="W,K", help="only the sweep of the two routes across m, for these row shapes (w static + k dynamic terms)")
args = ap.parse_args()
sys.path.insert(0, ROOT)
import numpy as np
import torch

import curve25519_dalek_amd as pkg

RAW, ED = 2, 0
E = pkg.engine
LANE, WAVE, AUTO = E.PRECOMP_ROWS_LANE, E.PRECOMP_ROWS_WAVE, E.PRECOMP_ROWS_AUTO
REPS, FEW_REPS, SLOW_MS = 11, 5, 100.0
PER_ROW_SAMPLE = 256
N_STATIC = 2050
POOL = 4096
SHAPES = [(4096, 130, 17), (256, 2050, 40), (1 << 17, 2, 1), (1 << 20, 1, 2), (64, 2048, 64), (4096, 2, 1)]
if args.quick:
    SHAPES = [(256, 130, 17), (4096, 2, 1)]
e = pkg.Engine(0)
g = torch.Generator(device="cuda"); g.manual_seed(17)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
fh = open(args.out, "w")


def out(s):
    print(s); sys.stdout.flush()
    fh.write(s + "\n"); fh.flush()


def timed(f, most=None):
    """-> (median, min, max) ms over REPS (FEW_REPS for a slow call; at most `most`) calls of f, events on the stream, after one warm-up call"""
    ts = []
    reps = most = most or REPS
    for k in range(REPS + 1):
        t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
        t0.record(); f(); t1.record(); t1.synchronize()
        if k == 0:                                           # the warm-up call decides how many follow
            reps = min(most, FEW_REPS if t0.elapsed_time(t1) > SLOW_MS else REPS)
            continue
        ts.append(t0.elapsed_time(t1))
        if len(ts) == reps:
            break
    return statistics.median(ts), min(ts), max(ts)


def fmt(t):
    return "%9.3f (%8.3f .. %9.3f)" % t


rng = np.random.default_rng(1)
pool = e.mul_base_batch(rng.integers(0, 256, (POOL, 32), dtype=np.uint8) & np.uint8(0x0F), RAW)
pool_dev = torch.from_numpy(pool).cuda()
handle = e.precomp_create(pool[:N_STATIC], in_fmt=RAW)


def scalars(*shape):
    s = torch.randint(0, 256, shape + (32,), device="cuda", generator=g, dtype=torch.uint8)
    s[..., 31] &= 0x0F
    return s.contiguous()


def per_row(ss, ds, dp, k):
    """-> (median, min, max) ms of ONE precomp_msm_vartime over the sample's rows, host clock"""
    ts = []
    e.precomp_msm_vartime(handle, ss[0], ds[:k], dp[:k], in_fmt=RAW)
    for r in range(ss.shape[0]):
        t0 = time.perf_counter()
        e.precomp_msm_vartime(handle, ss[r], ds[r * k:(r + 1) * k], dp[r * k:(r + 1) * k], in_fmt=RAW)
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def composition(ss, ds, dp, off):
    a = e.precomp_msm_vartime_rows_t(handle, ss, AUTO, RAW)
    st, b, ok = e.msm_vartime_segments_t(ds, dp, off, RAW, RAW)
    st2, o, ok2 = e.point_add_batch_t(a, b, in_fmt=RAW, out_fmt=ED)
    assert st == 0 and st2 == 0
    return o


def inputs(m, w, k):
    ss = scalars(m, w)
    ds = scalars(m * k)
    dp = pool_dev[torch.randint(0, POOL, (m * k,), device="cuda", generator=g)].contiguous()
    return ss, ds, dp, (np.arange(m + 1, dtype=np.uint64) * np.uint64(k))


def sweep(w, k, ms):
    """the two routes across m for one row shape: where they cross"""
    for m in ms:
        ss, ds, dp, off = inputs(m, w, k)
        res = {}
        lane = timed(lambda: res.__setitem__("lane", e.precomp_msm_vartime_mixed_rows_t(handle, ss, ds, dp, off, RAW, LANE, ED)), FEW_REPS)
        wave = timed(lambda: res.__setitem__("wave", e.precomp_msm_vartime_mixed_rows_t(handle, ss, ds, dp, off, RAW, WAVE, ED)), FEW_REPS)
        assert res["lane"][0] == 0 and torch.equal(res["lane"][1], res["wave"][1]), "the two routes disagree at %d x (%d + %d)" % (m, w, k)
        auto = "lane" if e.precomp_msm_vartime_mixed_rows_plan(m, w, off)[0] == LANE else "wave"
        fast = "lane" if lane[0] < wave[0] else "wave"
        out("   m %7d w %3d k %3d | lane %s | wave %s | faster route: %s x%.2f (AUTO: %s)"
            % (m, w, k, fmt(lane), fmt(wave), fast, max(lane[0], wave[0]) / min(lane[0], wave[0]), auto))


def shape(m, w, k, repeats=3):
    ss, ds, dp, off = inputs(m, w, k)
    sample = min(m, PER_ROW_SAMPLE)
    ss_h, ds_h, dp_h = ss[:sample].cpu().numpy(), ds[:sample * k].cpu().numpy(), dp[:sample * k].cpu().numpy()
    plan = e.precomp_msm_vartime_mixed_rows_plan(m, w, off)
    auto = "lane" if plan[0] == LANE else "wave"
    out("-- %d rows x (%d static + %d dynamic): AUTO takes the %s route, %d waves, %d pass(es) of at most %d dynamic terms" % ((m, w, k, auto) + plan[1:]))
    res, rows = {}, []
    for _ in range(repeats):
        lane = timed(lambda: res.__setitem__("lane", e.precomp_msm_vartime_mixed_rows_t(handle, ss, ds, dp, off, RAW, LANE, ED)))
        comp = timed(lambda: res.__setitem__("comp", composition(ss, ds, dp, off)))
        wave = timed(lambda: res.__setitem__("wave", e.precomp_msm_vartime_mixed_rows_t(handle, ss, ds, dp, off, RAW, WAVE, ED)))
        one = tuple(x * m for x in per_row(ss_h, ds_h, dp_h, k))
        assert res["lane"][0] == 0 and res["wave"][0] == 0 and bool(res["lane"][2].all()) and bool(res["wave"][2].all())
        assert torch.equal(res["lane"][1], res["wave"][1]), "the two routes disagree at %d x (%d + %d)" % (m, w, k)
        assert torch.equal(res["comp"], res["wave"][1]), "the mixed rows call and the composition disagree at %d x (%d + %d)" % (m, w, k)
        out("   lane %s | wave %s | composition %s | per row x m %s | faster route: %s"
            % (fmt(lane), fmt(wave), fmt(comp), "%11.3f (%10.3f .. %11.3f)" % one, "lane" if lane[0] < wave[0] else "wave"))
        rows.append({"lane": lane, "wave": wave, "comp": comp, "per_row": one})
    med = {key: [r[key][0] for r in rows] for key in ("lane", "wave", "comp", "per_row")}
    med["auto"] = med[auto]
    other = "wave" if auto == "lane" else "lane"
    for key, name in ((other, "the %s route" % other), ("comp", "the three-call composition"), ("per_row", "one precomp_msm_vartime per row")):
        lo, hi = (med["auto"], med[key])
        margin = min(hi) - max(lo) if statistics.median(hi) >= statistics.median(lo) else min(lo) - max(hi)
        spread = max(max(hi) - min(hi), max(lo) - min(lo))
        ratio = statistics.median(med[key]) / statistics.median(med["auto"])
        verdict = "LEVEL within the spread" if margin <= spread else ("AUTO faster x%.2f" % ratio if ratio > 1 else "AUTO SLOWER x%.2f" % (1 / ratio))
        out("   AUTO (%s) %.3f .. %.3f ms, %s %.3f .. %.3f ms: margin %.3f ms, spread of the medians %.3f ms -> %s"
            % (auto, min(med["auto"]), max(med["auto"]), name, min(med[key]), max(med[key]), margin, spread, verdict))


out("multiplier probe (Engine.microbench(0, 4000), best of 100): %.1f Top/s" % (max(e.microbench(0, 4000) for _ in range(100)) / 1e3))
out("precomp_msm_vartime_mixed_rows over %d static points, ms per call: median (min .. max) of %d calls (%d where a call takes more than %d ms); "
    "LANE_WIDTH %d, LANE_MIN_ROWS %d, DIRECT_MAX %d; per row: the median of at most %d single calls times m"
    % (N_STATIC, REPS, FEW_REPS, SLOW_MS, E.PRECOMP_ROWS_LANE_WIDTH, E.PRECOMP_ROWS_LANE_MIN_ROWS, E.MSM_SEGMENT_DIRECT_MAX, PER_ROW_SAMPLE))
e.precomp_msm_vartime_rows_t(handle, scalars(1, 1), WAVE, ED)       # (builds the comb table of the shared handle)
for m, w, k in ([] if args.sweep else SHAPES):
    shape(m, w, k)
out("-- the two routes across m, rows of w static + k dynamic terms: median (min .. max) of %d calls" % FEW_REPS)
SWEEP = [(1, 1), (2, 1), (1, 2), (2, 3), (4, 4), (8, 8), (15, 1), (15, 16), (2, 24), (2, 32), (15, 32), (2, 48), (2, 64), (15, 64)]
if args.sweep:
    SWEEP = [tuple(int(x) for x in item.split(",")) for item in args.sweep]
for w, k in ([(2, 1)] if args.quick else SWEEP):
    sweep(w, k, [1024, 4096] if args.quick else [1 << j for j in range(9, 18)])
e.precomp_destroy(handle)
fh.close()
