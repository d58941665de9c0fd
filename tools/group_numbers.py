#!/usr/bin/env python3
"""Group-law rates quoted in DESIGN.md / README.md / INTEGRATION.md that bench.py does not print (run on the GPU box): GPU time of the
whole call on device-resident points (torch tensors, events on the stream) at 2^20 and 2^24 items for add (RAW160 -> RAW160 and
CompressedEdwardsY -> CompressedEdwardsY), eq (RAW160, Edwards group) and the segmented sum (one segment, all segments of length 1,
random lengths 0 .. 3 C), each beside its model bound: bytes moved over the HBM bandwidth for the elementwise calls, additions over the
v_mad_u64_u32 rate (the box's multiplier probe) for the sum.  Then small batches through the host-pointer entry points against one CPU
core running the serial C restatement of the reference (oracle/): the crossover sets the shim's size threshold.
    python tools/group_numbers.py   (writes profiles/group_numbers.txt and prints it)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import curve25519_dalek_amd as pkg
from oracle import orc

e = pkg.Engine(0)
g = torch.Generator(device="cuda"); g.manual_seed(7)
lines = []
HBM = 8.0e12                 # MI355X HBM3E peak, bytes/s
MADS_PER_ADD = 9 * 100       # ge_add: 9 field multiplications of 10 x 10 limb products (v_mad_u64_u32 each)
C = 512                      # points per chunk of the segmented sum (SUM_C)


def out(s):
    print(s); sys.stdout.flush()
    lines.append(s)


def warm():
    for _ in range(40):
        e.microbench(0, 4000)


def best_dev(f, reps=5):
    warm(); f(); b = 1e9
    for _ in range(reps):
        t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
        t0.record(); f(); t1.record(); t1.synchronize()
        b = min(b, t0.elapsed_time(t1))
    return b


probe = max(e.microbench(0, 4000) for _ in range(60))          # Gop/s
out("multiplier probe (v_mad_u64_u32): %.1f Gop/s; HBM model %.1f TB/s; %d v_mad_u64_u32 per addition" % (probe, HBM / 1e12, MADS_PER_ADD))
table = torch.from_numpy(e.mul_base_batch(np.random.default_rng(1).integers(0, 256, (256, 32), dtype=np.uint8) & np.uint8(0x0F), 2)).cuda()
table_c = torch.from_numpy(e.compress_batch(table.cpu().numpy(), 0)).cuda()
out("%-44s %6s %10s %10s %10s" % ("", "n", "dev ms", "bound ms", "ratio"))
for lg in (20, 24):
    n = 1 << lg
    j = torch.randint(0, 256, (n,), device="cuda", generator=g)
    k = torch.randint(0, 256, (n,), device="cuda", generator=g)
    p, q = table[j].contiguous(), table[k].contiguous()
    ms = best_dev(lambda: e.point_add_batch_t(p, q, 0, 2, 2))
    bound = n * 480 / HBM * 1e3
    out("%-44s %6s %10.3f %10.3f %10.2f" % ("add RAW160 -> RAW160", "2^%d" % lg, ms, bound, ms / bound))
    pc, qc = table_c[j].contiguous(), table_c[k].contiguous()
    ms = best_dev(lambda: e.point_add_batch_t(pc, qc, 0, 0, 0))
    bound = n * 2 * 280 * 100 / (probe * 1e9) * 1e3          # two decompressions of ~280 multiplications each dominate
    out("%-44s %6s %10.3f %10.3f %10.2f" % ("add compressed -> compressed (bound: 2 decodes)", "2^%d" % lg, ms, bound, ms / bound))
    ms = best_dev(lambda: e.point_eq_batch_t(p, q, 2, 0))
    bound = n * 322 / HBM * 1e3
    out("%-44s %6s %10.3f %10.3f %10.2f" % ("eq RAW160, Edwards group", "2^%d" % lg, ms, bound, ms / bound))
    del pc, qc, q
    rng = np.random.default_rng(lg)
    cs = np.cumsum(rng.integers(0, 3 * C + 1, size=2 * n // (3 * C) + 16))
    off_r = np.concatenate([[0], cs[cs < n], [n]]).astype(np.int64)
    shapes = [("sum, one segment", torch.tensor([0, n], dtype=torch.int64, device="cuda")),
              ("sum, all segments of length 1", torch.arange(n + 1, dtype=torch.int64, device="cuda")),
              ("sum, random lengths 0 .. 3C (%d segments)" % (len(off_r) - 1), torch.from_numpy(off_r).cuda())]
    bound = n * MADS_PER_ADD / (probe * 1e9) * 1e3
    for name, off in shapes:
        ms = best_dev(lambda: e.point_sum_segments_t(p, off, 2, 2))
        out("%-44s %6s %10.3f %10.3f %10.2f" % (name, "2^%d" % lg, ms, bound, ms / bound))
    del p


def med(f, reps=21):
    f(); t = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); t.append((time.perf_counter() - t0) * 1e6)
    return sorted(t)[reps // 2]


def cpu_add(a, b):
    for i in range(a.shape[0]):
        orc.ed_compress(orc.ed_add(orc.ed_decompress(a[i].tobytes()), orc.ed_decompress(b[i].tobytes())))


def cpu_sum(a):
    acc = orc.ed_identity()
    for i in range(a.shape[0]):
        acc = orc.ed_add(acc, orc.ed_decompress(a[i].tobytes()))
    orc.ed_compress(acc)


tc = table_c.cpu().numpy()
warm()
out("small batches, host pointers, CompressedEdwardsY in and out, median of 21 calls (us): GPU call vs one CPU core (oracle/)")
out("%8s %12s %12s %12s %12s" % ("n", "add GPU", "add CPU", "sum GPU", "sum CPU"))
for m in (1, 4, 16, 64, 256, 1024, 4096):
    a = tc[np.arange(m) % 256].copy(); b = tc[(np.arange(m) * 7 + 3) % 256].copy()
    off = np.array([0, m], np.uint64)
    out("%8d %12.1f %12.1f %12.1f %12.1f" % (m, med(lambda: e.point_add_batch(a, b, 0, 0, 0)), med(lambda: cpu_add(a, b), 5),
                                             med(lambda: e.point_sum_segments(a, off, 0, 0)), med(lambda: cpu_sum(a), 5)))
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "group_numbers.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
