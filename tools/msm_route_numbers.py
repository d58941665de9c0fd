#!/usr/bin/env python3
"""What an outsider can see of the path a call takes: for each shape ONE call, then the name of its accumulation kernel (c25519_last_kernel_name), whether the
record was published by the path's last kernel (the change of Engine.counter(2)), the pass count of last_call_phase_ms and the status.  Two commits route alike
if their outputs are equal line for line (profiles/msm_route_numbers.txt).  The tool calls only entry points older than c25519_msm_route, but engine.py binds
every export of its own commit when it loads a library: to compare with a commit that lacks one, copy this file into a checkout of that commit and run it there.
--lib selects another build of THIS commit's sources (the tuning or debug build).

    python3 tools/msm_route_numbers.py [--lib path/to/libc25519hip_tune.so] [--out file]
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MSM_SIZES = [1, 1024, 4095, 4096, 6143, 6144, 8192, 1 << 18, (1 << 18) + 1, (1 << 18) + 2]
VERIFY_SIZES = [128, 129, 2047, 2048]
VERIFY_DEVICE_Z_SIZES = [65536, 65537]


def observe(eng, call):
    before = eng.counter(2)
    res = call()
    st, out = res if isinstance(res, tuple) else (res, b"")
    name = eng.lib.c25519_last_kernel_name(eng.ctx, 0).decode().split(" ")[0]
    return "kernel %-28s published %d passes %d status %d%s" % (name, eng.counter(2) - before, eng.last_call_phase_ms(0)[1], st,
                                                              (" result " + hashlib.sha256(out).hexdigest()[:12]) if out else "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import curve25519_dalek_amd as pkg
    if a.lib:
        pkg.select_library(a.lib)
    import torch
    eng = pkg.Engine(0)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    for n in MSM_SIZES:
        g = torch.Generator(device="cuda"); g.manual_seed(4100 + n)
        dx = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
        dx[:, 31] &= 0x0F
        for fmt, fname in ((2, "raw"), (0, "edwards_y")):
            dp = eng.mul_base_batch_t(dx, out_fmt=fmt)
            emit("msm %-9s n %6d device  %s" % (fname, n, observe(eng, lambda: eng.msm_vartime_t(dx, dp, in_fmt=fmt, out_fmt=0))))
            hx, hp = dx.cpu().numpy(), dp.cpu().numpy()
            emit("msm %-9s n %6d host    %s" % (fname, n, observe(eng, lambda: eng.msm_vartime(hx, hp, in_fmt=fmt, out_fmt=0))))
    for n in VERIFY_SIZES + VERIFY_DEVICE_Z_SIZES:
        g = torch.Generator(device="cuda"); g.manual_seed(4200 + n)
        seeds = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
        off = np.arange(n + 1, dtype=np.int64) * 32
        dm = torch.randint(0, 256, (32 * n,), dtype=torch.uint8, device="cuda", generator=g)
        doff = torch.from_numpy(off).cuda()
        dpk, dsig = eng.sign_batch_t(seeds, dm, doff)
        for z_mode in ((1,) if n in VERIFY_DEVICE_Z_SIZES else (1, 0)):
            emit("verify z_mode %d n %6d device  %s" % (z_mode, n, observe(eng, lambda: eng.verify_batch_t(dm, doff, dsig, dpk, z_mode))))
            if n in VERIFY_DEVICE_Z_SIZES:
                continue
            hm, hs, hk = dm.cpu().numpy().tobytes(), dsig.cpu().numpy(), dpk.cpu().numpy()
            M = [hm[32 * i:32 * i + 32] for i in range(n)]; S = [hs[i].tobytes() for i in range(n)]; K = [hk[i].tobytes() for i in range(n)]
            emit("verify z_mode %d n %6d host    %s" % (z_mode, n, observe(eng, lambda: eng.verify_batch(M, S, K, z_mode))))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
