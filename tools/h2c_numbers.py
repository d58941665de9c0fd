#!/usr/bin/env python3
"""Hash-to-group rates quoted in DESIGN.md / README.md that bench.py does not print (run on the GPU box): whole-call time and items/s
at 2^16 and 2^20 items of from_uniform_bytes (-> CompressedRistretto and -> RAW160), hash_from_bytes of 32-byte messages and the
RFC 9380 Edwards hash_to_curve (RO, the RFC's DST), device-resident (torch tensors, GPU time of the whole call on the stream) and
host-pointer (numpy in / out, wall clock).  X25519 2^20 as the yardstick, and the box's multiplier-probe reading first.
    python tools/h2c_numbers.py > profiles/h2c_numbers.txt"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import curve25519_dalek_amd as pkg
import devlib; devlib.apply(pkg)

E = pkg.engine
DST = b"QUUX-V01-CS02-with-edwards25519_XMD:SHA-512_ELL2_RO_"
e = pkg.Engine(0)
g = torch.Generator(device="cuda"); g.manual_seed(7)


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


print("multiplier probe (v_mad_u64_u32): %.1f Gop/s" % max(e.microbench(0, 4000) for _ in range(60)))
k = rnd(1 << 20); u = rnd(1 << 20)
ms = best_dev(lambda: e.x25519_batch_t(k, u))
print("x25519 2^20, device-resident (yardstick): %.3f ms  %.2f M/s" % (ms, (1 << 20) / ms / 1e3))
print("%-44s %8s %12s %12s %12s" % ("", "n", "dev ms", "dev M/s", "host ms"))
for lg in (16, 20):
    n = 1 << lg
    a64 = rnd(n, 64); a64h = a64.cpu().numpy()
    m32 = rnd(n, 32).reshape(-1); off = torch.arange(0, 32 * (n + 1), 32, dtype=torch.int64, device="cuda")
    msgs_h = [bytes(r) for r in m32.reshape(n, 32).cpu().numpy()]
    blob_h, off_h = e._pack(msgs_h)
    outs = {f: np.empty((n, 160 if f == 2 else 32), np.uint8) for f in (0, 1, 2)}
    rows = [
        ("from_uniform_bytes -> RISTRETTO", lambda: e.ristretto_from_uniform_bytes_batch_t(a64, 1),
         lambda: e.ristretto_from_uniform_bytes_batch(a64h, 1, out=outs[1])),
        ("from_uniform_bytes -> RAW160", lambda: e.ristretto_from_uniform_bytes_batch_t(a64, 2),
         lambda: e.ristretto_from_uniform_bytes_batch(a64h, 2, out=outs[2])),
        ("hash_from_bytes 32-byte msgs -> RISTRETTO", lambda: e.ristretto_hash_from_bytes_batch_t(m32, off, 1),
         lambda: e.ristretto_hash_from_bytes_batch(blob_h, 1, msg_off=off_h, out=outs[1])),
        ("Edwards hash_to_curve RO 32-byte -> EDWARDS_Y", lambda: e.edwards_hash_to_curve_batch_t(m32, off, DST, E.H2C_RO, 0),
         lambda: e.edwards_hash_to_curve_batch(blob_h, DST, E.H2C_RO, 0, msg_off=off_h, out=outs[0])),
        ("Edwards hash_to_curve RO 32-byte -> RAW160", lambda: e.edwards_hash_to_curve_batch_t(m32, off, DST, E.H2C_RO, 2),
         lambda: e.edwards_hash_to_curve_batch(blob_h, DST, E.H2C_RO, 2, msg_off=off_h, out=outs[2])),
    ]
    for name, fd, fh in rows:
        d = best_dev(fd); h = best_host(fh)
        print("%-44s %8s %12.3f %12.2f %12.3f" % (name, "2^%d" % lg, d, n / d / 1e3, h))
        sys.stdout.flush()
