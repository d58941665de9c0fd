#!/usr/bin/env python3
"""MontgomeryPoint rates quoted in DESIGN.md / README.md that bench.py does not print (run on the GPU box): GPU time of the whole call
at 2^20 device-resident items (torch tensors, events on the stream) of Mul<&Scalar>, mul_bits_be at nbits = 255 and 512, mul_base
(constant-time and vartime tables) and to_edwards (-> compressed, -> RAW160), with X25519 2^20 in the same run as the yardstick, the
box's multiplier-probe reading first, and the host-pointer wall clock of each.  Then the A/B of to_edwards' division: the batched
division of k_ratio_p32 (the default) against one fe_invert per lane (C25519_MONT_TO_EDWARDS_BATCHED=0), each arm in a fresh child
process on the tuning build.
    python tools/montgomery_numbers.py   (writes profiles/montgomery_numbers.txt and prints it)"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import curve25519_dalek_amd as pkg

CHILD = len(sys.argv) > 1 and sys.argv[1] == "--to-edwards-arm"
if CHILD:
    pkg.select_library(os.path.join(ROOT, "curve25519-dalek_amd", "lib", "libc25519hip_tune.so"))
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


n = 1 << 20
u = rnd(n); k = rnd(n)
s = rnd(n); s[:, 31] &= 0x0F                                       # canonical scalars for mul_base
sg = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
uc = torch.from_numpy(e.to_montgomery_batch(e.mul_base_batch(s.cpu().numpy(), 2))).cuda()   # u of curve points: to_edwards succeeds
if CHILD:
    ms = best_dev(lambda: e.montgomery_to_edwards_batch_t(uc, sg, 0))
    print("CHILD %.3f" % ms)
    sys.exit(0)

out("multiplier probe (v_mad_u64_u32): %.1f Gop/s" % max(e.microbench(0, 4000) for _ in range(60)))
x_ms = best_dev(lambda: e.x25519_batch_t(k, u))
out("x25519 2^20, device-resident (yardstick, k_x25519 + k_ratio_p32): %.3f ms  %.2f M/s" % (x_ms, n / x_ms / 1e3))
b255 = rnd(n, 32)[:, :32].contiguous()
b512 = rnd(n, 64)
vt = pkg.Engine(0, flags=pkg.engine.FLAG_VARTIME_TABLES)
kh, uh, sh, uch, sgh = k.cpu().numpy(), u.cpu().numpy(), s.cpu().numpy(), uc.cpu().numpy(), sg.cpu().numpy()
b255h, b512h = b255.cpu().numpy(), b512.cpu().numpy()
o32, o160 = np.empty((n, 32), np.uint8), np.empty((n, 160), np.uint8)
rows = [
    ("Mul<&Scalar> (k_mont_mul)", lambda: e.montgomery_mul_batch_t(k, u), lambda: e.montgomery_mul_batch(kh, uh, out=o32)),
    ("mul_bits_be, nbits 255", lambda: e.montgomery_mul_bits_be_batch_t(b255, 255, u), lambda: e.montgomery_mul_bits_be_batch(b255h, 255, uh, out=o32)),
    ("mul_bits_be, nbits 512", lambda: e.montgomery_mul_bits_be_batch_t(b512, 512, u), lambda: e.montgomery_mul_bits_be_batch(b512h, 512, uh, out=o32)),
    ("mul_base (constant-time tables)", lambda: e.montgomery_mul_base_batch_t(s), lambda: e.montgomery_mul_base_batch(sh, out=o32)),
    ("mul_base (vartime tables)", lambda: vt.montgomery_mul_base_batch_t(s), lambda: vt.montgomery_mul_base_batch(sh, out=o32)),
    ("to_edwards -> compressed", lambda: e.montgomery_to_edwards_batch_t(uc, sg, 0), lambda: e.montgomery_to_edwards_batch(uch, sgh, 0, out=o32)),
    ("to_edwards -> RAW160", lambda: e.montgomery_to_edwards_batch_t(uc, sg, 2), lambda: e.montgomery_to_edwards_batch(uch, sgh, 2, out=o160)),
]
out("%-40s %8s %12s %12s %12s %10s" % ("", "n", "dev ms", "dev M/s", "host ms", "/ x25519"))
res = {}
for name, fd, fh in rows:
    dm = best_dev(fd); hm = best_host(fh)
    res[name] = dm
    out("%-40s %8s %12.3f %12.2f %12.3f %10.3f" % (name, "2^20", dm, n / dm / 1e3, hm, dm / x_ms))
x2 = best_dev(lambda: e.x25519_batch_t(k, u))
out("x25519 2^20 again at the end: %.3f ms" % x2)
del vt
# small batches through the host-pointer entry points (what a shim calls) against the serial C restatement of the reference (oracle/, one
# core): the crossover sets the shim's size threshold.  CPU ladder: orc.x25519_batch (the same 255 steps);
# CPU to_edwards: orc.fe_invert + orc.ed_decompress per item through ctypes (an upper bound by the call overhead, ~1 us per item)
sys.path.insert(0, ROOT)
from oracle import orc


def med(f, reps=21):
    f(); t = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); t.append((time.perf_counter() - t0) * 1e6)
    return sorted(t)[reps // 2]


def cpu_to_edwards(ub, sgb):
    for i in range(ub.shape[0]):
        uu = int.from_bytes(ub[i].tobytes(), "little") & (2**255 - 1)
        y = orc.fe_mul(((uu - 1) % (2**255 - 19)).to_bytes(32, "little"), orc.fe_invert(((uu + 1) % (2**255 - 19)).to_bytes(32, "little")))
        yb = bytearray(y); yb[31] ^= (int(sgb[i]) << 7) & 0xFF
        orc.ed_decompress(bytes(yb))


warm()
out("small batches, host pointers, median of 21 calls (us): GPU call vs one CPU core (oracle/)")
out("%8s %14s %14s %16s %16s" % ("n", "mul GPU", "ladder CPU", "to_edwards GPU", "to_edwards CPU"))
for m in (1, 4, 16, 64, 256, 1024, 4096):
    kk, uu_, cc, ss = kh[:m].copy(), uh[:m].copy(), uch[:m].copy(), sgh[:m].copy()
    out("%8d %14.1f %14.1f %16.1f %16.1f" % (m, med(lambda: e.montgomery_mul_batch(kk, uu_)), med(lambda: orc.x25519_batch(kk, uu_, threads=1), 5),
                                             med(lambda: e.montgomery_to_edwards_batch(cc, ss, 0)), med(lambda: cpu_to_edwards(cc, ss), 5)))
# the A/B of the division in to_edwards, each arm a fresh process on the tuning build
failed = False
for arm in ("0", "1"):
    env = dict(os.environ, C25519_MONT_TO_EDWARDS_BATCHED=arm)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--to-edwards-arm"], capture_output=True, text=True, timeout=600, env=env)
    ms = [l for l in r.stdout.split("\n") if l.startswith("CHILD ")]
    if r.returncode != 0 or not ms:
        out("to_edwards A/B arm %s failed: rc %d %s" % (arm, r.returncode, r.stderr[-400:]))
        failed = True
        break
    out("to_edwards -> compressed, tuning build, %-34s %8.3f ms" % ("per-lane fe_invert (knob 0):" if arm == "0" else "batched division (default):",
                                                                     float(ms[0].split()[1])))
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "montgomery_numbers.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
sys.exit(1 if failed else 0)
