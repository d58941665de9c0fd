#!/usr/bin/env python3
"""The segmented verify_batch (ed25519_verify_batch_segments_dev) against the two routes a caller with many independent batches had before it, on one
box in one run (run on the GPU box): 2^16 honest signatures over 32-byte messages, device-resident, cut into segments of 1, 4, 16, 64, 256 and 1023
signatures.
    new   one ed25519_verify_batch_segments_dev call
    (a)   one ed25519_verify_batch_keys_dev call per segment, one after the other as a caller would issue them (every call synchronises, so the
          calls do not overlap); timed on the first A_SAMPLE segments and scaled to m
    (b)   one ed25519_verify_each_dev over all 2^16 signatures: per-signature verdicts, no batching
(a) and (b) are code the segmented call does not change.  Device z-mode with the keys' cached points and with key bytes; the transcript z-mode (one
Merlin transcript per segment: on the device up to ED25519_TRANSCRIPT_SEGMENT_DEVICE_MAX signatures, on the host beyond) in rows of its own.  After a warm-up run of every arm the three
arms ALTERNATE, REPS rounds in one process; each figure is the median with (min .. max) beside it, and a difference within the spreads is a tie.  The
statuses of the new call are checked to be all OK at every shape, and with one forged signature per 97 segments against the positions forged.
Then the break-even: the smallest number of segments m (powers of two) from which the new call beats (a), per length; 2^20 signatures in segments
of 4, 64 and 256 (several passes of the segmented MSM); and a proxy for what the call's second synchronisation costs.
    python tools/verify_seg_numbers.py [--out FILE]
(writes profiles/verify_seg_numbers.txt of this tree, or FILE, and prints it)

The transcript z-mode's own arms -- where the Merlin transcripts of the segments run -- are a run of their own:
    python tools/verify_seg_numbers.py --transcript-arms host=LIB:0 device=LIB:1023 [parent=OTHERLIB] [--reps 7]
Every arm is a build of the library (LIB: lib/libc25519hip_tune.so; OTHERLIB: e.g. the release library of the parent commit) on a context of its own in this
one process; ":K" sets the tuning knob C25519_VSEG_TRANSCRIPT_DEV_MAX of that arm to K (0: every transcript on the host, 1023: every one on the device) --
the knob is read once per loaded file, so each such arm loads a private copy of the file; "@LABEL" behind a spec is printed in place of the file's path.  Same signatures, same shapes, cached key points; the arms ALTERNATE
within every round.  Then the kernel alone (ed25519_batch_transcript_zs_segments_dev on device-resident hashes: wall clock around the call and a
synchronisation, and the events of c25519_last_kernel_ms) and the break-even number of segments of 4, 64 and 256 signatures between the first two arms.
This run REPLACES the part of the output file from the line "== transcript z-mode: where the transcripts run" on and keeps what is above it."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_seg_numbers.txt"))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--transcript-arms", nargs="+", metavar="NAME=LIB[:DEV_MAX][@LABEL]", default=None)
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
if args.transcript_arms:
    NBIG = N                                                # (this run needs no more)
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


TR_MARK = "== transcript z-mode: where the transcripts run"


def transcript_arms(specs):
    import ctypes as C
    import shutil
    import tempfile
    vp, u64 = C.c_void_p, C.c_uint64
    tmp = tempfile.mkdtemp(prefix="vseg_arms_")
    stream = torch.cuda.current_stream().cuda_stream
    mlen = N * MSG

    def call(arm, off, msgs_t=msgs):
        name, lib, ctx = arm
        m, n = off.shape[0] - 1, int(off[-1])
        status = torch.empty((m,), dtype=torch.uint8, device="cuda")
        st = lib.ed25519_verify_batch_segments_dev(ctx, msgs_t.data_ptr(), moff.data_ptr(), n * MSG, sigs.data_ptr(), pks.data_ptr(), points.data_ptr(), n,
                                                   off.ctypes.data, m, 0, status.data_ptr())
        assert st == 0, (name, st, lib.c25519_last_error(ctx))
        return status

    arms, shown = [], []
    for spec in specs:
        name, _, rest = spec.partition("=")
        rest, _, label = rest.partition("@")
        path, _, knob = rest.partition(":")
        shown.append("%s=%s%s" % (name, label or path, ":" + knob if knob else ""))
        path = os.path.abspath(path)
        os.environ.pop("C25519_VSEG_TRANSCRIPT_DEV_MAX", None)
        if knob:
            private = os.path.join(tmp, name + ".so")
            shutil.copy(path, private)
            path = private
            os.environ["C25519_VSEG_TRANSCRIPT_DEV_MAX"] = knob
        lib = C.CDLL(path)
        lib.c25519_ctx_create.restype, lib.c25519_ctx_create.argtypes = vp, [C.c_int, C.c_uint32]
        lib.c25519_ctx_set_stream.argtypes = [vp, vp]
        lib.c25519_last_error.restype, lib.c25519_last_error.argtypes = C.c_char_p, [vp]
        lib.ed25519_verify_batch_segments_dev.restype = C.c_int32
        lib.ed25519_verify_batch_segments_dev.argtypes = [vp, vp, vp, u64, vp, vp, vp, u64, vp, u64, C.c_uint32, vp]
        ctx = lib.c25519_ctx_create(0, 0)
        assert ctx, spec
        lib.c25519_ctx_set_stream(ctx, stream)
        arms.append((name, lib, ctx))
        call(arms[-1], offsets(4, 16))                      # the arm's first call in this z-mode reads its knob: now, while the variable holds its value
    os.environ.pop("C25519_VSEG_TRANSCRIPT_DEV_MAX", None)
    shutil.rmtree(tmp, ignore_errors=True)                  # (the files stay mapped)
    names = [a[0] for a in arms]

    def rounds(off):
        ts = {nm: [] for nm in names}
        for _ in range(REPS):
            for a in arms:
                ts[a[0]].append(wall(lambda: call(a, off)))
        return {nm: stats(v) for nm, v in ts.items()}

    def versus(x, y, xn, yn):
        """x against y: by more than the larger of the two spreads, or a tie"""
        spread = max(x[2] - x[1], y[2] - y[1])
        if abs(x[0] - y[0]) <= spread:
            return "%s ~ %s (tie)" % (xn, yn)
        return "%s x%.2f faster than %s" % ((xn, y[0] / x[0], yn) if x[0] < y[0] else (yn, x[0] / y[0], xn))

    out(TR_MARK)
    out("arms: " + "; ".join(shown))
    out("-- ed25519_verify_batch_segments_dev, transcript z-mode, cached key points: ms per call, wall clock around the call and a device synchronisation, median (min .. max) of "
        "%d rounds in which the arms alternate; %d signatures of %d-byte messages" % (REPS, N, MSG))
    for ln in LENS:
        off = offsets(ln)
        m = off.shape[0] - 1
        warm()
        bad = torch.tensor([int(off[s]) * MSG + 3 for s in range(0, m, 97)], device="cuda")
        fm = msgs[:mlen].clone()
        fm[bad] ^= 1
        want = np.zeros(m, np.uint8); want[list(range(0, m, 97))] = 3
        for a in arms:
            assert not bool(call(a, off).any()), "an honest segment was rejected (%s)" % a[0]
            assert np.array_equal(call(a, off, fm).cpu().numpy(), want), "forged segments: wrong statuses (%s)" % a[0]
        r = rounds(off)
        row = "len %4d m %6d | " % (ln, m) + " | ".join("%s %s" % (nm, fmt(r[nm])) for nm in names)
        if len(names) >= 2:
            row += " | " + versus(r[names[1]], r[names[0]], names[1], names[0])
        if len(names) >= 3:
            row += " | " + versus(r[names[0]], r[names[2]], names[0], names[2])
        out(row)

    out("-- the kernel alone: ed25519_batch_transcript_zs_segments_dev of the release library on device-resident hashes (every segment on the device), ms: wall clock around the "
        "call and a synchronisation | its events (c25519_last_kernel_ms); the first and the last segment are compared with the host function")
    hram = e.batch_hram_t(msgs[:mlen], moff[:N + 1], sigs[:N], pks[:N])
    hh, hs = hram[:N * 64].reshape(N, 64).cpu().numpy(), sigs[:N].cpu().numpy()
    for ln, m in [(ln, None) for ln in LENS] + [(1023, 1), (4096, 1), (4096, 16)]:
        off = offsets(ln, m)
        m, n = off.shape[0] - 1, int(off[-1])
        hn, sn = hram[:n * 64], sigs[:n]
        z = e.batch_transcript_zs_segments_t(hn, sn, off).cpu().numpy()
        for a, b in ((0, ln), (n - ln, n)):
            assert np.array_equal(z[a:b], pkg.engine.batch_transcript_zs(hh[a:b], hs[a:b])), "the device transcript differs from the host's"
        tw, tk = [], []
        for _ in range(REPS):
            tw.append(wall(lambda: e.batch_transcript_zs_segments_t(hn, sn, off)))
            tk.append(e.last_kernel_ms())
        t0 = time.perf_counter()
        for s in range(min(m, 64)):
            pkg.engine.batch_transcript_zs(hh[s * ln:(s + 1) * ln], hs[s * ln:(s + 1) * ln])
        host_ms = (time.perf_counter() - t0) * 1e3 * m / min(m, 64)
        out("len %4d m %6d | wall %s | events %s | %.3f us per signature of a segment | the host function over the same segments, one after the other: %.3f ms"
            % (ln, m, fmt(stats(tw)), fmt(stats(tk)), statistics.median(tk) * 1e3 / ln, host_ms))

    if len(names) >= 2:
        out("-- break-even, %s against %s: m segments of one length (m a power of two), the smallest m from which %s is faster by more than the spread" % (names[1], names[0], names[1]))
        two = arms[:2]
        for ln in (4, 64, 256):
            found, m = None, 1
            while m * ln <= N:
                off = offsets(ln, m)
                ts = {two[0][0]: [], two[1][0]: []}
                for a in two:
                    call(a, off)
                for _ in range(REPS):
                    for a in two:
                        ts[a[0]].append(wall(lambda: call(a, off)))
                h, d = stats(ts[names[0]]), stats(ts[names[1]])
                out("len %4d m %6d | %s %s | %s %s | %s" % (ln, m, names[0], fmt(h), names[1], fmt(d), versus(d, h, names[1], names[0])))
                if found is None and d[0] < h[0] and abs(d[0] - h[0]) > max(h[2] - h[1], d[2] - d[1]):
                    found = m
                m *= 4 if m >= 64 else 2
            out("   len %d: %s wins from m = %s" % (ln, names[1], found if found is not None else "never at this size"))
    keep = []
    if os.path.exists(args.out):
        for l in open(args.out).read().split("\n"):
            if l.startswith(TR_MARK):
                break
            keep.append(l)
        while keep and not keep[-1]:
            keep.pop()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(keep + lines) + "\n")


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


if args.transcript_arms:
    transcript_arms(args.transcript_arms)
    sys.exit(0)
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
