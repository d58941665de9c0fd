"""The path a call takes on the GPU is the one its route names (csrc/msm.hip "routes", Engine.msm_route): at the boundaries between the small path, the mid
path and the bucket pipeline the result is right -- (sum x_i^2) B from the oracle for the MSM, honest signatures and one flipped bit for verify_batch -- and what
an outsider can see of the path agrees with the route: the name of the accumulation kernel, the pass count, and whether the record was published by the path's
last kernel (Engine.counter(2) advances by one)."""
import subprocess

import numpy as np
import pytest

import util
from test_gpu_msm import _sumsq_device, i2b

pytestmark = pytest.mark.gpu
OK, VERIFY = 0, 3
RAW, EDWARDS_Y = 2, 0
SMALL = "c25519::k_small_cols"
MSM_SIZES = [1, 1024, 4095, 4096, 6143, 6144, 8192, 1 << 18, (1 << 18) + 1, (1 << 18) + 2]


@pytest.fixture(scope="module")
def eng():
    import curve25519_dalek_amd as pkg
    return pkg.Engine(0)


def observed(eng, call):
    """-> (what the call returned, first word of the accumulation kernel's name, publications, pass count)"""
    before = eng.counter(2)
    res = call()
    name = eng.lib.c25519_last_kernel_name(eng.ctx, 0).decode()
    return res, name, eng.counter(2) - before, eng.last_call_phase_ms(0)[1]


def check_msm_signature(r, terms, raw, name, published, passes):
    assert published == (1 if r["publish"] else 0), (r, published)
    if r["path"] == "small":
        assert name.startswith("c25519::k_small_cols"), (r, name)
        assert passes == (0 if r["publish"] else 1)         # (the lean, directly published small call keeps no pass records)
    elif r["path"] == "mid":
        # raw points: the mid path's own accumulation; records: the one with the over-long lists in front up to 2^17 + 1 terms, the plain one above
        want = "c25519::k_mid_acc_long" if raw else "c25519::k_accumulate_long" if terms <= (1 << 17) + 1 else "c25519::k_accumulate "
        assert name.startswith(want), (r, name)
        assert passes == 0                                   # (no pass records for the MSM's own mid-size calls)
    else:
        assert name.startswith("c25519::k_accumulate "), (r, name)
        assert passes == r["passes"], (r, passes)


@pytest.mark.parametrize("n", MSM_SIZES)
def test_msm_takes_the_path_of_its_route(eng, orc, n):
    import torch
    import curve25519_dalek_amd as pkg
    g = torch.Generator(device="cuda"); g.manual_seed(7100 + n)
    dx = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
    dx[:, 31] &= 0x0F
    want = orc.ed_compress(orc.ed_mul_base(i2b(_sumsq_device(dx))))
    hx = dx.cpu().numpy()
    for fmt in (RAW, EDWARDS_Y):
        dp = eng.mul_base_batch_t(dx, out_fmt=fmt)
        hp = dp.cpu().numpy()
        for host in (False, True):
            call = (lambda: eng.msm_vartime(hx, hp, in_fmt=fmt, out_fmt=0)) if host else (lambda: eng.msm_vartime_t(dx, dp, in_fmt=fmt, out_fmt=0))
            (st, got), name, published, passes = observed(eng, call)
            assert st == OK and got == want, (n, fmt, host)
            r = pkg.Engine.msm_route(0, n, fmt, host)
            assert r["prep_points"] == (fmt != RAW)
            check_msm_signature(r, n, fmt == RAW, name, published, passes)


def _batch(eng, n, seed):
    import torch
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    seeds = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
    lens = [(7 * i) % 61 for i in range(n)]
    off = np.zeros(n + 1, dtype=np.int64); off[1:] = np.cumsum(lens)
    dm = torch.randint(0, 256, (max(int(off[-1]), 1),), dtype=torch.uint8, device="cuda", generator=g)
    doff = torch.from_numpy(off).cuda()
    dp, ds = eng.sign_batch_t(seeds, dm, doff)
    return dm, doff, off, ds, dp


def check_verify_signature(r, n, name, published):
    assert published == (1 if r["publish"] else 0), (r, published)
    if r["path"] == "small":
        assert name.startswith(SMALL), (r, name)
    elif r["path"] == "mid":
        assert name.startswith("c25519::k_accumulate_long" if 2 * n + 1 <= (1 << 17) + 1 else "c25519::k_accumulate "), (r, name)
    elif r["path"] == "pipeline":
        assert name.startswith("c25519::k_accumulate "), (r, name)


@pytest.mark.parametrize("n", [128, 129, 2047, 2048, 65536, 65537])
def test_verify_batch_takes_the_path_of_its_route(eng, orc, n):
    import curve25519_dalek_amd as pkg
    dm, doff, off, ds, dp = _batch(eng, n, 7200 + n)
    i = n // 2
    bad = ds.clone(); bad[i, 9] ^= 0x10
    m = dm[int(off[i]):int(off[i + 1])].cpu().numpy().tobytes()
    assert orc.ed25519_verify(dp[i].cpu().numpy().tobytes(), m, ds[i].cpu().numpy().tobytes()) == 0
    for z_mode in ((1,) if n > 2048 else (1, 0)):
        st, name, published, _ = observed(eng, lambda: eng.verify_batch_t(dm, doff, ds, dp, z_mode))
        assert st == OK, (n, z_mode)
        if z_mode == 1:                                      # (the route of the device z-mode; a transcript batch never publishes from the device-pointer call)
            check_verify_signature(pkg.Engine.msm_route(1, n), n, name, published)
        else:                                                # (the MSM's widths capped at 16: 6-bit windows up to 6143 terms, the small path)
            assert published == 0 and name.startswith(SMALL), (n, name)
        assert eng.verify_batch_t(dm, doff, bad, dp, z_mode) == VERIFY, (n, z_mode)
        if n > 2048:
            continue
        hm, hs, hk = dm.cpu().numpy().tobytes(), ds.cpu().numpy(), dp.cpu().numpy()
        M = [hm[int(off[k]):int(off[k + 1])] for k in range(n)]; S = [hs[k].tobytes() for k in range(n)]; K = [hk[k].tobytes() for k in range(n)]
        st, name, published, _ = observed(eng, lambda: eng.verify_batch(M, S, K, z_mode))
        assert st == OK, (n, z_mode)
        if n <= 128:                                         # verify_batch_small_host, either z-mode: the small path publishes the record
            assert published == 1 and name.startswith(SMALL), (n, z_mode, name, published)
        elif z_mode == 1:
            check_verify_signature(pkg.Engine.msm_route(1, n, host_pointers=True), n, name, published)
        else:
            assert published == 0 and name.startswith(SMALL), (n, name)
        Sb = list(S); Sb[i] = bad[i].cpu().numpy().tobytes()
        assert eng.verify_batch(M, Sb, K, z_mode) == VERIFY, (n, z_mode)


CHILD = r'''
import sys
sys.path.insert(0, %r)
import numpy as np, torch
import curve25519_dalek_amd as pkg
from oracle import orc
from test_gpu_msm import _sumsq_device, i2b
eng = pkg.Engine(0)
for n, path, passes in ((98304, "mid", 1), (98305, "pipeline", 2)):
    r = pkg.Engine.msm_route(0, n)
    assert (r["path"], r["passes"]) == (path, passes), r
    g = torch.Generator(device="cuda"); g.manual_seed(7300 + n)
    dx = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
    dx[:, 31] &= 0x0F
    dp = eng.mul_base_batch_t(dx, out_fmt=2)
    before = eng.counter(2)
    st, got = eng.msm_vartime_t(dx, dp, in_fmt=2, out_fmt=0)
    assert st == 0 and got == orc.ed_compress(orc.ed_mul_base(i2b(_sumsq_device(dx)))), n
    name = eng.lib.c25519_last_kernel_name(eng.ctx, 0).decode()
    seen = eng.last_call_phase_ms(0)[1]
    assert eng.counter(2) - before == (1 if r["publish"] else 0), (n, r)
    assert name.startswith("c25519::k_mid_acc_long" if path == "mid" else "c25519::k_accumulate "), (n, name)
    assert seen == (0 if path == "mid" else passes), (n, seen)
print("child route ok")
'''


def test_pass_size_knob_moves_the_split_on_the_gpu():
    """tuning build, C25519_MSM_PASS_LOG2 = 16: 98304 terms are one pass on the mid path, 98305 terms two passes on the bucket pipeline"""
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run(util.child_argv(CHILD % here), capture_output=True, text=True, timeout=600, env=util.tune_env({"C25519_MSM_PASS_LOG2": "16"}))
    assert out.returncode == 0 and "child route ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
