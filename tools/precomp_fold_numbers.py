#!/usr/bin/env python3
"""Many mixed multiscalar equations folded into ONE multiscalar mul (c25519_precomp_msm_vartime_mixed_rows_fold_dev) against what the parent
commit has for the same input, on one box (run on the GPU box): m rows of w static scalars over the first w of 2050 static points plus k
dynamic terms of their own, RAW160 dynamic points, 16-byte weights, CompressedEdwardsY out, everything device-resident.
    (a) fold        the fold call
    (b) mixed rows  c25519_precomp_msm_vartime_mixed_rows_dev on the same input (route AUTO): one point per row, what locates a bad row
    (c) MSM alone   the final MSM on pre-folded scalars: c25519_precomp_msm_vartime over w static scalars (host pointers: 32 w bytes go up) and
                    c25519_msm_vartime_dev over the m k dynamic terms, device-resident -- the two halves the fold call runs, without its kernels
    kernels         the fold kernels' own time, from the call's phase timers (c25519_phase_ms 0: the column fold, 1: the dynamic scaling)
Shapes (rows x (static + dynamic)): 4096 x (130 + 17), 256 x (2050 + 40), 131072 x (2 + 1), 2^20 x (1 + 2), 64 x (2 + 1).  All three calls
synchronise before they return, so each figure is the HOST clock around the call: the median of REPS calls (FEW_REPS where one takes longer
than SLOW_MS) after a warm-up call of the same shape, min .. max beside it.  Every shape is timed three times over, the calls alternating:
the larger spread of two sides' three medians is what a margin has to exceed.  The fold's result is checked against Python integers fed to
c25519_precomp_msm_vartime wherever m (w + k) <= 2^20.  Last, (a) and (b) across m = 1 .. 64 for the first and the third row shape: the
smallest m from which the fold is the faster call.
Every shape runs in a process of its own under a time limit of its own (--limit seconds); after one that fails or runs out of time nothing
more is started.
    python tools/precomp_fold_numbers.py [--out FILE] [--quick] [--limit SECONDS]
(writes profiles/precomp_fold_numbers.txt, or FILE, and prints it as it goes)"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "precomp_fold_numbers.txt"))
ap.add_argument("--quick", action="store_true", help="small shapes only (to try the script)")
ap.add_argument("--limit", type=int, default=240, help="seconds one step may take")
ap.add_argument("--step", help="(internal) run one step in this process: head | shape:m,w,k | sweep:w,k")
args = ap.parse_args()

SHAPES = [(4096, 130, 17), (256, 2050, 40), (1 << 17, 2, 1), (1 << 20, 1, 2), (64, 2, 1)]
SWEEPS = [(130, 17), (2, 1)]
if args.quick:
    SHAPES, SWEEPS = [(256, 130, 17), (64, 2, 1)], [(2, 1)]

if not args.step:
    # the parent: starts the steps one after the other, each under its time limit, and never opens the GPU itself
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    steps = ["head"] + ["shape:%d,%d,%d" % s for s in SHAPES] + ["sweep:%d,%d" % s for s in SWEEPS]
    with open(args.out, "w") as fh:
        for step in steps:
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], capture_output=True, text=True, timeout=args.limit)
                text, rc = p.stdout, p.returncode
                if rc:
                    text += p.stderr[-2000:]
            except subprocess.TimeoutExpired as ex:
                text, rc = (ex.stdout or b"").decode() if isinstance(ex.stdout, bytes) else (ex.stdout or ""), 124
            print(text, end=""); sys.stdout.flush()
            fh.write(text); fh.flush()
            if rc:
                msg = "step %s ended with status %d: nothing more is started\n" % (step, rc)
                print(msg, end=""); fh.write(msg)
                sys.exit(1)
    sys.exit(0)

sys.path.insert(0, ROOT)
import numpy as np
import torch

import curve25519_dalek_amd as pkg

RAW, ED = 2, 0
E = pkg.engine
L = 2**252 + 27742317777372353535851937790883648493
REPS, FEW_REPS, SLOW_MS = 11, 5, 100.0
N_STATIC = 2050
POOL = 4096
e = pkg.Engine(0)
g = torch.Generator(device="cuda"); g.manual_seed(17)


def out(s):
    print(s); sys.stdout.flush()


def timed(f, most=None):
    """-> (median, min, max) ms over REPS (FEW_REPS for a slow call; at most `most`) calls of f, host clock (f synchronises), after one warm-up call"""
    ts = []
    reps = most = most or REPS
    for k in range(REPS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); f(); dt = (time.perf_counter() - t0) * 1e3
        if k == 0:                                           # the warm-up call decides how many follow
            reps = min(most, FEW_REPS if dt > SLOW_MS else REPS)
            continue
        ts.append(dt)
        if len(ts) == reps:
            break
    return statistics.median(ts), min(ts), max(ts)


def fmt(t):
    return "%8.3f (%8.3f .. %8.3f)" % t


if args.step == "head":
    out("multiplier probe (Engine.microbench(0, 4000), best of 100): %.1f Top/s" % (max(e.microbench(0, 4000) for _ in range(100)) / 1e3))
    out("precomp_msm_vartime_mixed_rows_fold over %d static points, 16-byte weights, ms per call on the host clock (every call synchronises): median "
        "(min .. max) of %d calls (%d where a call takes more than %d ms)" % (N_STATIC, REPS, FEW_REPS, SLOW_MS))
    sys.exit(0)

rng = np.random.default_rng(1)
pool = e.mul_base_batch(rng.integers(0, 256, (POOL, 32), dtype=np.uint8) & np.uint8(0x0F), RAW)
pool_dev = torch.from_numpy(pool).cuda()
handle = e.precomp_create(pool[:N_STATIC], in_fmt=RAW)


def scalars(*shape):
    s = torch.randint(0, 256, shape + (32,), device="cuda", generator=g, dtype=torch.uint8)
    s[..., 31] &= 0x0F                                       # (the mixed rows call refuses bit 255; the fold would take any value)
    return s.contiguous()


def inputs(m, w, k):
    ss = scalars(m, w)
    ds = scalars(m * k)
    dp = pool_dev[torch.randint(0, POOL, (m * k,), device="cuda", generator=g)].contiguous()
    wt = torch.randint(0, 256, (m, 16), device="cuda", generator=g, dtype=torch.uint8).contiguous()
    return ss, ds, dp, (np.arange(m + 1, dtype=np.uint64) * np.uint64(k)), wt


def check(m, w, k, ss, ds, dp, wt, got):
    """the fold against Python integers fed to the single call"""
    ints = lambda a: [int.from_bytes(bytes(r), "little") for r in a.cpu().numpy().reshape(-1, a.shape[-1])]
    S, D, Wt = ints(ss), ints(ds), ints(wt)
    t = [sum(Wt[r] * S[r * w + j] for r in range(m)) % L for j in range(w)]
    d = [Wt[i // k] * D[i] % L for i in range(m * k)]
    tob = lambda v: np.frombuffer(b"".join(x.to_bytes(32, "little") for x in v), np.uint8).reshape(-1, 32)
    st, want = e.precomp_msm_vartime(handle, tob(t), tob(d), dp.cpu().numpy(), in_fmt=RAW, out_fmt=ED)
    assert st == 0 and got == want, "the fold differs from the single call on (t, d') at %d x (%d + %d)" % (m, w, k)


def shape(m, w, k, repeats=3):
    ss, ds, dp, off, wt = inputs(m, w, k)
    plan = e.precomp_msm_vartime_mixed_rows_fold_plan(m, w, off)
    out("-- %d rows x (%d static + %d dynamic): one MSM of %d static + %d dynamic terms; the column fold in %d slice(s) of %d rows" % ((m, w, k) + plan))
    t_pre, d_pre = scalars(w).cpu().numpy(), scalars(m * k)                          # pre-folded scalars: canonical values of the same sizes
    none32, none160 = np.zeros((0, 32), np.uint8), np.zeros((0, 160), np.uint8)

    def msm_alone():
        e.precomp_msm_vartime(handle, t_pre, none32, none160, in_fmt=RAW, out_fmt=RAW)
        e.msm_vartime_t(d_pre, dp, RAW, ED)

    res, rows = {}, []
    for _ in range(repeats):
        fold = timed(lambda: res.__setitem__("fold", e.precomp_msm_vartime_mixed_rows_fold_t(handle, ss, ds, dp, off, wt, RAW, ED)))
        kern = (e.phase_ms(0, 0), e.phase_ms(0, 1))
        mixed = timed(lambda: res.__setitem__("mixed", e.precomp_msm_vartime_mixed_rows_t(handle, ss, ds, dp, off, RAW, E.PRECOMP_ROWS_AUTO, ED)))
        alone = timed(msm_alone)
        assert res["fold"][0] == 0 and res["mixed"][0] == 0
        out("   (a) fold %s | (b) mixed rows %s | (c) MSM alone %s | fold kernels: columns %.3f + dynamic %.3f" % (fmt(fold), fmt(mixed), fmt(alone), kern[0], kern[1]))
        rows.append({"fold": fold, "mixed": mixed, "alone": alone, "kern": kern})
    if m * (w + k) <= 1 << 20:
        check(m, w, k, ss, ds, dp, wt, res["fold"][1])
        out("   the fold equals c25519_precomp_msm_vartime on (t, d') from Python integers")
    med = {key: [r[key][0] for r in rows] for key in ("fold", "mixed", "alone")}
    lo, hi = med["fold"], med["mixed"]
    margin = min(hi) - max(lo) if statistics.median(hi) >= statistics.median(lo) else min(lo) - max(hi)
    spread = max(max(hi) - min(hi), max(lo) - min(lo))
    ratio = statistics.median(hi) / statistics.median(lo)
    verdict = "LEVEL within the spread" if margin <= spread else ("fold faster x%.2f" % ratio if ratio > 1 else "fold SLOWER x%.2f" % (1 / ratio))
    out("   (a) %.3f .. %.3f ms, (b) %.3f .. %.3f ms: margin %.3f ms, spread of the medians %.3f ms -> %s" % (min(lo), max(lo), min(hi), max(hi), margin, spread, verdict))
    a, c = statistics.median(med["fold"]), statistics.median(med["alone"])
    kk = statistics.median([sum(r["kern"]) for r in rows])
    out("   (a) - (c) = %.3f ms = %.0f %% of (a); the fold kernels themselves %.3f ms = %.0f %% of (a)" % (a - c, 100 * (a - c) / a, kk, 100 * kk / a))


def sweep(w, k):
    """(a) and (b) across small m: from where the fold is the faster call"""
    out("-- (a) against (b) across m, rows of %d static + %d dynamic terms: median (min .. max) of %d calls" % (w, k, FEW_REPS))
    first, prev_faster = None, False
    for m in (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64):
        ss, ds, dp, off, wt = inputs(m, w, k)
        fold = timed(lambda: e.precomp_msm_vartime_mixed_rows_fold_t(handle, ss, ds, dp, off, wt, RAW, ED), FEW_REPS)
        mixed = timed(lambda: e.precomp_msm_vartime_mixed_rows_t(handle, ss, ds, dp, off, RAW, E.PRECOMP_ROWS_AUTO, ED), FEW_REPS)
        faster = fold[0] < mixed[0]
        if faster and not prev_faster:
            first = m
        prev_faster = faster
        out("   m %4d | (a) fold %s | (b) mixed rows %s | %s" % (m, fmt(fold), fmt(mixed), "fold faster x%.2f" % (mixed[0] / fold[0]) if faster else "mixed rows faster x%.2f" % (fold[0] / mixed[0])))
    out("   the fold is the faster call from m = %s on (of the m tried), and at every larger m tried" % first if prev_faster and first is not None
        else "   the fold is not the faster call at the largest m tried")


e.precomp_msm_vartime_rows_t(handle, scalars(1, 1), E.PRECOMP_ROWS_WAVE, ED)       # (builds the comb table of the mixed rows call: not part of any figure)
kind, _, rest = args.step.partition(":")
nums = tuple(int(x) for x in rest.split(","))
if kind == "shape":
    shape(*nums)
else:
    sweep(*nums)
e.precomp_destroy(handle)
