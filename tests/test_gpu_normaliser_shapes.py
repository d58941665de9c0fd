"""The MSM's normaliser k_prep_raw2 (csrc/msm.hip: raw points -> affine records, one inversion per lane; a lane whose points all have Z literally 1 skips it) in
its general form at CH = 4, 16, 32 and 64 points per lane and in its speculative-affine form (SPEC, the cached key points of verify_batch), with affine and
projective points mixed by wave, by chain step, by lane and singly.  The sum is the observable: one wrong record changes it.

Where the general form still runs in the release library: raw MSMs beyond 2^18 + 1 terms (below, the small and mid paths take raw points as they are), and
wherever prep_points is called directly -- the dynamic part of precomp_msm_vartime at any size (CH = 4 below 2^18 points)."""
import random

import numpy as np
import pytest

import pyref_finish as F
import util
from test_gpu_msm import _sumsq_device, i2b, rows

pytestmark = pytest.mark.gpu
P = F.P
OK, VERIFY = 0, 3
RAW160 = 2
MASKS = ("all_projective", "all_affine", "alternate_waves", "alternate_steps", "every_third", "first_projective", "last_projective")


@pytest.fixture(scope="module")
def eng():
    import curve25519_dalek_amd as pkg
    return pkg.Engine(0)


def prep_ch(n):
    """points per lane of the general normaliser for a launch over n points (msm.hip prep_points_on)"""
    return 64 if n >= 1 << 23 else 32 if n >= 1 << 20 else 16 if n >= 1 << 18 else 4


def affine_mask(name, n, launches, xp=np):
    """True where the point is given in affine form (Z literally 1).  launches: [(first point, points, T)] of the normaliser's launches -- only the chain-step
    mask looks at it; the others do not know the geometry and stay meaningful if it changes."""
    i = xp.arange(n)
    if name == "all_projective":
        return i < 0
    if name == "all_affine":
        return i >= 0
    if name == "alternate_waves":
        return (i // 64) % 2 == 1
    if name == "every_third":
        return i % 3 != 0
    if name == "first_projective":
        return i != 0
    if name == "last_projective":
        return i != n - 1
    assert name == "alternate_steps"
    m = i < 0
    for lo, cnt, T in launches:
        m = m | ((i >= lo) & (i < lo + cnt) & (((i - lo) // T) % 2 == 1))
    return m


# ---- 1. the general form at CH = 4: the dynamic part of precomp_msm_vartime ---------------------------------------------------------------
DYN_SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1027, 4099]


@pytest.fixture(scope="module")
def dyn(eng):
    n = max(DYN_SIZES)
    proj = eng.mul_base_batch(util.rand_scalars(7701, n), out_fmt=RAW160)
    st, aff, ok = eng.decompress_batch(eng.compress_batch(proj))
    assert st == 0 and ok.all()
    one = np.zeros(40, np.uint8); one[0] = 1
    assert (aff[:, 80:120] == one).all() and (proj[:, 80:120] == one).all(axis=1).mean() < 0.01      # Z literally 1 / (all but never) not 1
    h = eng.precomp_create(eng.mul_base_batch(util.rand_scalars(7702, 1), out_fmt=RAW160), in_fmt=RAW160)
    yield util.rand_scalars(7703, n), proj, aff, h
    eng.precomp_destroy(h)


@pytest.mark.parametrize("n", DYN_SIZES)
def test_dynamic_terms_of_precomp_msm_mixed_affine_and_projective(eng, orc, dyn, n):
    """n <= 1024: one to four steps at T = 256 with whole waves out of range and the clamped last block; 1025: the grid grows to 512 lanes"""
    x, proj, aff, h = dyn
    T = F.chain_T(n, ch=prep_ch(n))
    assert prep_ch(n) == 4 and T == 256 * -(-n // 1024)
    want = orc.ed_compress(orc.ed_msm(rows(x[:n]), rows(proj[:n])))
    e32 = np.zeros((0, 32), np.uint8)
    for name in MASKS:
        pts = np.where(affine_mask(name, n, [(0, n, T)])[:, None], aff[:n], proj[:n])
        st, got = eng.precomp_msm_vartime(h, e32, x[:n], pts, in_fmt=RAW160)
        assert st == 0 and got == want, (n, name)


# ---- 2. the release pipeline: CH = 16, 32, 64 ---------------------------------------------------------------------------------------------
def prep_launches(n):
    """[(first point, points, CH)] of the normaliser's launches for a raw MSM of n points on the bucket pipeline (msm.hip msm_record_enqueue): a single pass
    prepares its own points; of several passes the first prepares its own and the second those of ALL later passes in one launch"""
    import curve25519_dalek_amd as pkg
    r = pkg.Engine.msm_route(0, n, RAW160)
    assert r["path"] == "pipeline", r
    if r["passes"] == 1:
        return [(0, n, prep_ch(n))]
    return [(0, r["per"], prep_ch(r["per"])), (r["per"], n - r["per"], prep_ch(n - r["per"]))]


# the points per lane each size selects.  (2^23 + 193 points are five passes: no launch of the normaliser sees 2^23 points, so CH = 64 needs the larger size.)
PIPELINE_SIZES = {(1 << 18) + 64 * 37 + 3: [16], (1 << 20) + 64 * 5 + 1: [32], (1 << 23) + 64 * 3 + 1: [32, 32], (1 << 23) + (1 << 21) + 64 * 3 + 1: [32, 64]}


@pytest.mark.parametrize("n", list(PIPELINE_SIZES))
def test_pipeline_msm_mixed_affine_and_projective(eng, orc, n):
    import torch
    launches = prep_launches(n)
    assert [ch for _, _, ch in launches] == PIPELINE_SIZES[n]
    g = torch.Generator(device="cuda"); g.manual_seed(7800 + n % 1000)
    dx = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
    dx[:, 31] &= 0x0F
    want = orc.ed_compress(orc.ed_mul_base(i2b(_sumsq_device(dx))))
    proj = eng.mul_base_batch_t(dx, out_fmt=RAW160)
    st, aff, ok = eng.decompress_batch_t(eng.compress_batch_t(proj))
    assert st == 0 and bool(ok.all())
    one = torch.zeros(40, dtype=torch.uint8, device="cuda"); one[0] = 1
    assert bool((aff[:, 80:120] == one).all()) and float((proj[:, 80:120] == one).all(dim=1).float().mean()) < 0.01
    geo = [(lo, cnt, F.chain_T(cnt, ch=ch)) for lo, cnt, ch in launches]
    for name in MASKS:
        pts = torch.where(affine_mask(name, n, geo, xp=_TorchIdx(torch))[:, None], aff, proj)
        st, got = eng.msm_vartime_t(dx, pts, in_fmt=RAW160, out_fmt=0)
        assert st == 0 and got == want, (n, name)
        # the records came from the normaliser: the bucket pipeline's accumulation, not the mid path's (which reads raw points)
        assert eng.lib.c25519_last_kernel_name(eng.ctx, 0).decode().startswith("c25519::k_accumulate "), (n, name)


class _TorchIdx:
    """arange on the device for affine_mask"""

    def __init__(self, torch):
        self.torch = torch

    def arange(self, n):
        return self.torch.arange(n, device="cuda")


# ---- 3. the speculative-affine form: verify_batch with cached key points ------------------------------------------------------------------
def spec_ch(n):
    return 8 if n >= 1 << 18 else 4


def placements(n, T):
    """name -> indices of the key points to give in projective form.  A wave is 64 consecutive lanes; it returns early iff every point of its chains has Z = 1."""
    waves = list(range(0, min(n, T), 64))
    every = []
    for k, w0 in enumerate(waves):
        t = w0 + k % 64 if w0 + k % 64 < n else w0
        every.append(t + (k % F.chain_len(n, T, t)) * T)
    last77 = 77 + (F.chain_len(n, T, 77) - 1) * T
    return {"first_wave": [T + 5 if T + 5 < n else 5], "last_partial_wave": [n - 1], "every_wave": every, "chain_ends": [77, last77]}


@pytest.mark.parametrize("n", [1024, 1025, 4099, (1 << 18) + 65])
def test_verify_batch_cached_key_points_scaled_in_places(eng, orc, n):
    import torch
    from test_gpu_msm_route import _batch
    rnd = random.Random(7900 + n)
    dm, doff, off, ds, dp = _batch(eng, n, 7900 + n % 1000)
    hm = dm.cpu().numpy().tobytes()
    for i in (0, 1, n // 2, n - 2, n - 1):                   # honest signatures, by the oracle
        assert orc.ed25519_verify(dp[i].cpu().numpy().tobytes(), hm[int(off[i]):int(off[i + 1])], ds[i].cpu().numpy().tobytes()) == 0, i
    st, dpts, ok = eng.decompress_batch_t(dp)
    assert st == 0 and bool(ok.all())
    hp = dpts.cpu().numpy()
    T = F.chain_T(n, ch=spec_ch(n))
    waves = set(range(0, min(n, T), 64))

    def flipped(i):
        bad = ds.clone(); bad[i, 9] ^= 0x10
        return bad

    assert eng.verify_batch_t(dm, doff, ds, dp, 1, pk_points=dpts) == OK
    assert eng.verify_batch_t(dm, doff, flipped(n // 3), dp, 1, pk_points=dpts) == VERIFY
    for name, idx in placements(n, T).items():
        assert all(0 <= i < n for i in idx), (name, idx)
        pts = hp.copy()
        for i in idx:
            pts[i] = F.to_raw160([F.scale(F.parse_raw160(hp[i:i + 1])[0], rnd.randrange(2, P))])[0]
        dpk = torch.from_numpy(pts).cuda()
        assert eng.verify_batch_t(dm, doff, ds, dp, 1, pk_points=dpk) == OK, (n, name)
        late = {(i % T) // 64 * 64 for i in idx}            # the waves that go on to the general algorithm
        assert eng.verify_batch_t(dm, doff, flipped(min(late) + 1 if min(late) + 1 < n else min(late)), dp, 1, pk_points=dpk) == VERIFY, (n, name)
        early = sorted(waves - late)
        assert bool(early) == (name != "every_wave"), (n, name)
        if early:                                            # a signature whose key's record the early-returning pass wrote
            assert eng.verify_batch_t(dm, doff, flipped(early[-1] + 3 if early[-1] + 3 < n else early[-1]), dp, 1, pk_points=dpk) == VERIFY, (n, name)
