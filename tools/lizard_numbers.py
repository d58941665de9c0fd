#!/usr/bin/env python3
"""Lizard rates quoted in DESIGN.md / README.md that bench.py does not print (run on the GPU box): whole-call time and items/s at
2^16 and 2^20 items of lizard_encode::<Sha256> (-> CompressedRistretto and -> RAW160), lizard_decode::<Sha256> (from
CompressedRistretto and from RAW160) and map_to_curve_inverse (from CompressedRistretto), device-resident (torch tensors, GPU time
of the whole call on the stream) and host-pointer (numpy in / out, wall clock).  The decode inputs are real Lizard encodings.
X25519 2^20 as the yardstick on the same box, and the box's multiplier-probe reading first.
    python tools/lizard_numbers.py   (writes profiles/lizard_numbers.txt and prints it)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import curve25519_dalek_amd as pkg

e = pkg.Engine(0)
g = torch.Generator(device="cuda"); g.manual_seed(7)
lines = []


def out(s):
    print(s); sys.stdout.flush()
    lines.append(s)


def rnd(n, w=32):
    return torch.randint(0, 256, (n, w), dtype=torch.uint8, device="cuda", generator=g)


def warm():
    for _ in range(40):
        e.microbench(0, 4000)             # sustained clock first (see bench.py)


def best_dev(f, reps=5):
    warm(); f(); b = 1e9
    for _ in range(reps):
        t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
        t0.record(); f(); t1.record(); t1.synchronize()
        b = min(b, t0.elapsed_time(t1))
    return b


def best_host(f, reps=3):
    warm(); f(); b = 1e9
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter(); f(); b = min(b, (time.perf_counter() - t0) * 1e3)
    return b


out("multiplier probe (v_mad_u64_u32): %.1f Gop/s" % max(e.microbench(0, 4000) for _ in range(60)))
k = rnd(1 << 20); u = rnd(1 << 20)
x_ms = best_dev(lambda: e.x25519_batch_t(k, u))
out("x25519 2^20, device-resident (yardstick): %.3f ms  %.2f M/s" % (x_ms, (1 << 20) / x_ms / 1e3))
del k, u
out("%-40s %8s %12s %12s %12s" % ("", "n", "dev ms", "dev M/s", "host ms"))
for lg in (16, 20):
    n = 1 << lg
    d = rnd(n, 16); dh = d.cpu().numpy()
    enc = e.ristretto_lizard_encode_batch_t(d, 1); raw = e.ristretto_lizard_encode_batch_t(d, 2)
    st = e.ristretto_lizard_decode_batch_t(enc, 1)[1]
    assert bool((st == 1).all())
    ench, rawh = enc.cpu().numpy(), raw.cpu().numpy()
    # host outputs reused across calls, as a caller should (a fresh array pays first-touch page faults inside the copy: ffi.h)
    o32, o160, o16, ost, o512 = np.empty((n, 32), np.uint8), np.empty((n, 160), np.uint8), np.empty((n, 16), np.uint8), np.empty((n,), np.uint8), np.empty((n, 16, 32), np.uint8)
    rows = [
        ("lizard_encode -> RISTRETTO", lambda: e.ristretto_lizard_encode_batch_t(d, 1), lambda: e.ristretto_lizard_encode_batch(dh, 1, out=o32)),
        ("lizard_encode -> RAW160", lambda: e.ristretto_lizard_encode_batch_t(d, 2), lambda: e.ristretto_lizard_encode_batch(dh, 2, out=o160)),
        ("lizard_decode <- RISTRETTO", lambda: e.ristretto_lizard_decode_batch_t(enc, 1), lambda: e.ristretto_lizard_decode_batch(ench, 1, out=o16, status=ost)),
        ("lizard_decode <- RAW160", lambda: e.ristretto_lizard_decode_batch_t(raw, 2), lambda: e.ristretto_lizard_decode_batch(rawh, 2, out=o16, status=ost)),
        ("map_to_curve_inverse <- RISTRETTO", lambda: e.ristretto_map_to_curve_inverse_batch_t(enc, 1),
         lambda: e.ristretto_map_to_curve_inverse_batch(ench, 1, out=o512)),
    ]
    for name, fd, fh in rows:
        dm = best_dev(fd); hm = best_host(fh)
        out("%-40s %8s %12.3f %12.2f %12.3f" % (name, "2^%d" % lg, dm, n / dm / 1e3, hm))
        if lg == 20 and name == "lizard_decode <- RISTRETTO":
            dec_ms = dm
out("decode 2^20 (compressed) / X25519 2^20 time: %.2f" % (dec_ms / x_ms))
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "lizard_numbers.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
