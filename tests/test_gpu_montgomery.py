"""MontgomeryPoint on the GPU (csrc/montgomery.hip): Mul<&Scalar>, mul_bits_be, mul_base and to_edwards, through dalek.*, Engine
(host twins and device tensors) and plain C, against the reference's cases (tests/golden/montgomery_vectors.json), the big-integer
restatement tests/pyref_montgomery.py, the X25519 entry points and the Edwards fixed-base path."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import pyref as R
import pyref_montgomery as M
import util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = json.load(open(os.path.join(ROOT, "tests", "golden", "montgomery_vectors.json")))
LIBDIR = os.path.join(ROOT, "curve25519-dalek_amd", "lib")
P = M.P
NINE = bytes([9]) + bytes(31)


@pytest.fixture(scope="module")
def eng():
    import curve25519_dalek_amd as pkg
    return pkg.Engine(0)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def _rows(a):
    return [bytes(a[i]) for i in range(a.shape[0])]


def _arr(items, width=32):
    return np.frombuffer(b"".join(items), np.uint8).reshape(-1, width).copy()


def _clamp(k):
    b = bytearray(k)
    b[0] &= 248; b[31] &= 127; b[31] |= 64
    return bytes(b)


def _low_order_us(golden):
    return [golden.bytes("src/constants.rs", "X25519_LOW_ORDER_POINTS", i) for i in range(7)]


# ---- the reference's cases ------------------------------------------------------------------------------------------
def test_golden_cases_through_dalek(eng):
    from curve25519_dalek_amd import dalek
    cases = VEC["to_edwards"]
    got = dalek.MontgomeryPoint.to_edwards([bytes.fromhex(u) for u, _, _ in cases], [s for _, s, _ in cases], engine=eng)
    assert got == [bytes.fromhex(w) if w is not None else None for _, _, w in cases]
    a, b = (bytes.fromhex(x) for x in VEC["eq_defined_mod_p"])
    k = bytes(range(32))
    ra, rb = dalek.MontgomeryPoint.mul([a, b], [k, k], engine=eng)
    assert ra == rb == M.mul(a, k)
    lad = VEC["ladder_matches_edwards"]
    assert dalek.MontgomeryPoint.mul([bytes.fromhex(u) for u, _, _ in lad], [bytes.fromhex(s) for _, s, _ in lad], engine=eng) == \
        [bytes.fromhex(w) for _, _, w in lad]
    # mul_base_clamped / mul_clamped are the X25519 paths; mul_bits_be of the 255 scalar bits is mul
    raw = [bytes([0xFF] * 32), bytes(range(1, 33))]
    assert dalek.MontgomeryPoint.mul_base_clamped(raw, engine=eng) == dalek.MontgomeryPoint.mul_clamped([NINE, NINE], raw, engine=eng)
    s = bytes.fromhex(lad[0][1])
    assert dalek.MontgomeryPoint.mul_bits_be([NINE], [M.scalar_bits_be(s)], engine=eng) == dalek.MontgomeryPoint.mul([NINE], [s], engine=eng)
    assert dalek.MontgomeryPoint.mul_base([s], engine=eng) == dalek.MontgomeryPoint.mul([NINE], [s], engine=eng)


# ---- the ladder --------------------------------------------------------------------------------------------------------
def test_mul_random_vs_pyref(eng):
    rng = random.Random(81)
    n = 1 << 12
    ks = [rng.randbytes(32) for _ in range(n)]
    us = [rng.randbytes(32) for _ in range(n)]
    ks[:16] = [b"\xff" * 32] * 16                         # all ones (bit 255 set, and skipped)
    ks[16:32] = [bytes(31) + b"\x80"] * 16                # only bit 255: the ladder sees zero -> identity -> u = 0
    got = _rows(eng.montgomery_mul_batch(_arr(ks), _arr(us)))
    assert got == [M.mul(u, k) for k, u in zip(ks, us)]
    assert all(g == bytes(32) for g in got[16:32])
    # bit 255 of the scalar is ignored
    k2 = _arr(ks); k2[:, 31] ^= 0x80
    assert _rows(eng.montgomery_mul_batch(k2, _arr(us))) == got


def test_mul_non_canonical_and_small_order_u(eng, golden):
    rng = random.Random(82)
    us = [(P + i).to_bytes(32, "little") for i in range(19)]                                 # p .. 2^255 - 1: non-canonical
    us += [bytes(b[:31]) + bytes([b[31] | 0x80]) for b in (rng.randbytes(32) for _ in range(40))]    # bit 255 set
    us += _low_order_us(golden) + [(2).to_bytes(32, "little"), (P - 1).to_bytes(32, "little")]          # small order; the twist
    us += [rng.randbytes(32) for _ in range(60)]
    ks = [rng.randbytes(32) for _ in us]
    got = _rows(eng.montgomery_mul_batch(_arr(ks), _arr(us)))
    assert got == [M.mul(u, k) for k, u in zip(ks, us)]
    # a clamped scalar kills the small-order component: all zero, as X25519 gives
    lo = _low_order_us(golden)
    assert not eng.montgomery_mul_batch(_arr([_clamp(k) for k in ks[:7]]), _arr(lo)).any()


def test_mul_of_clamped_scalars_is_x25519_2p20(eng, torch):
    n = 1 << 20
    g = torch.Generator(device="cuda"); g.manual_seed(83)
    k = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
    u = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
    kc = k.clone()
    kc[:, 0] &= 248; kc[:, 31] &= 127; kc[:, 31] |= 64
    got = eng.montgomery_mul_batch_t(kc, u)
    want = eng.x25519_batch_t(k, u)
    assert torch.equal(got, want)


# ---- mul_bits_be -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbits", [0, 1, 7, 8, 255, 256, 300, 512])
def test_mul_bits_be_vs_pyref(eng, nbits):
    rng = random.Random(84 + nbits)
    n = 96
    bits = [[rng.getrandbits(1) for _ in range(nbits)] for _ in range(n)]
    if nbits:
        bits[0] = [1] * nbits
        bits[1] = [0] * nbits
    us = [rng.randbytes(32) for _ in range(n)]
    packed = np.packbits(np.array(bits, dtype=bool).reshape(n, nbits), axis=1) if nbits else np.empty((n, 0), np.uint8)
    got = _rows(eng.montgomery_mul_bits_be_batch(packed, nbits, _arr(us)))
    assert got == [M.mul_bits_be(u, b) for u, b in zip(us, bits)]
    if nbits == 0:
        assert all(g == bytes(32) for g in got)
    if nbits % 8:                                          # the padding bits of the last byte are ignored
        p2 = packed.copy(); p2[:, -1] |= (1 << (8 - nbits % 8)) - 1
        assert _rows(eng.montgomery_mul_bits_be_batch(p2, nbits, _arr(us))) == got


def test_mul_bits_be_255_is_mul(eng):
    rng = np.random.default_rng(85)
    n = 4096
    k = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    u = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    # bits 254..0 of k, MSB first: the 256 bits big-endian without the first
    be = np.unpackbits(k[:, ::-1], axis=1)[:, 1:]
    packed = np.packbits(be, axis=1)
    assert np.array_equal(eng.montgomery_mul_bits_be_batch(packed, 255, u), eng.montgomery_mul_batch(k, u))


# ---- mul_base ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vartime", [False, True])
def test_mul_base_matches_ladder_and_to_montgomery(vartime):
    import curve25519_dalek_amd as pkg
    e = pkg.Engine(0, flags=pkg.engine.FLAG_VARTIME_TABLES if vartime else 0)
    s = util.rand_scalars(86, 5000)
    s[:2] = 0; s[1, 0] = 1
    got = e.montgomery_mul_base_batch(s)
    assert np.array_equal(got, e.montgomery_mul_batch(s, np.tile(np.frombuffer(NINE, np.uint8), (s.shape[0], 1))))
    assert np.array_equal(got, e.to_montgomery_batch(e.mul_base_batch(s, out_fmt=2)))
    assert got[0].tobytes() == bytes(32) and got[1].tobytes() == NINE
    assert [got[i].tobytes() for i in range(2, 12)] == [M.mul_base(s[i].tobytes()) for i in range(2, 12)]


# ---- to_edwards --------------------------------------------------------------------------------------------------------
def _check_to_edwards(eng, us, signs):
    out, st = eng.montgomery_to_edwards_batch(_arr(us), np.array(signs, np.uint8), 0)
    raw, st2 = eng.montgomery_to_edwards_batch(_arr(us), np.array(signs, np.uint8), 2)
    assert np.array_equal(st, st2)
    for i, (u, sg) in enumerate(zip(us, signs)):
        pt = M.to_edwards_point(u, sg)
        assert int(st[i]) == (pt is not None), (u.hex(), sg)
        if pt is None:
            assert not out[i].any() and not raw[i].any()
        else:
            assert out[i].tobytes() == R.ed_compress(pt), (u.hex(), sg)
            assert M.raw160_affine(raw[i].tobytes()) == pt, (u.hex(), sg)
    return st


def test_to_edwards_special_u_and_signs(eng, golden):
    us = [bytes(32), (1).to_bytes(32, "little"), (P - 1).to_bytes(32, "little"), (2).to_bytes(32, "little"), NINE] + _low_order_us(golden)
    signs = [0, 1, 2, 3, 128, 129, 255]
    uu = [u for u in us for _ in signs]
    ss = [s for _ in us for s in signs]
    st = _check_to_edwards(eng, uu, ss)
    # u = 0 with sign 1: "negative zero" -- x stays 0, the encoding is y = -1 without the sign bit, the point is (0, -1)
    out, _ = eng.montgomery_to_edwards_batch(_arr([bytes(32)]), np.array([1], np.uint8), 0)
    assert out[0].tobytes() == (P - 1).to_bytes(32, "little")
    raw, _ = eng.montgomery_to_edwards_batch(_arr([bytes(32)]), np.array([1], np.uint8), 2)
    assert M.raw160_affine(raw[0].tobytes()) == (0, P - 1)
    # u = -1 and u = 2 are rejected for every sign
    assert not st[2 * len(signs):4 * len(signs)].any()


def test_to_edwards_statuses_on_a_half_twist_mix(eng):
    rng = random.Random(87)
    us = [rng.randbytes(32) for _ in range(3000)]
    signs = [rng.randrange(256) for _ in us]
    st = _check_to_edwards(eng, us, signs)
    assert 1200 < int(st.sum()) < 1800                    # about half of random u are on the twist


def test_to_edwards_round_trip_2p18(eng):
    n = 1 << 18
    s = util.rand_scalars(88, n)
    raw = eng.mul_base_batch(s, out_fmt=2)
    comp = eng.compress_batch(raw, 0)
    u = eng.to_montgomery_batch(raw)
    sign = comp[:, 31] >> 7
    out, st = eng.montgomery_to_edwards_batch(u, sign, 0)
    assert st.all() and np.array_equal(out, comp)
    out2, st2 = eng.montgomery_to_edwards_batch(u, sign, 2)
    assert st2.all() and np.array_equal(eng.compress_batch(out2, 0), comp)


# ---- entry points ------------------------------------------------------------------------------------------------------
def test_device_and_host_forms_agree(eng, torch):
    rng = np.random.default_rng(89)
    n = 3000
    k = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    u = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    sg = rng.integers(0, 256, size=(n,), dtype=np.uint8)
    kt, ut, st_ = (torch.from_numpy(x).cuda() for x in (k, u, sg))
    assert np.array_equal(eng.montgomery_mul_batch_t(kt, ut).cpu().numpy(), eng.montgomery_mul_batch(k, u))
    bits = rng.integers(0, 256, size=(n, 38), dtype=np.uint8)
    assert np.array_equal(eng.montgomery_mul_bits_be_batch_t(torch.from_numpy(bits).cuda(), 300, ut).cpu().numpy(),
                          eng.montgomery_mul_bits_be_batch(bits, 300, u))
    assert np.array_equal(eng.montgomery_mul_bits_be_batch_t(None, 0, ut).cpu().numpy(), np.zeros((n, 32), np.uint8))
    assert np.array_equal(eng.montgomery_mul_base_batch_t(kt).cpu().numpy(), eng.montgomery_mul_base_batch(k))
    for fmt in (0, 2):
        o, s = eng.montgomery_to_edwards_batch_t(ut, st_, fmt)
        ho, hs = eng.montgomery_to_edwards_batch(u, sg, fmt)
        assert np.array_equal(o.cpu().numpy(), ho) and np.array_equal(s.cpu().numpy(), hs)


def test_bad_arguments_and_empty(eng):
    import curve25519_dalek_amd as pkg
    E = pkg.engine
    z = np.zeros((1, 32), np.uint8)
    with pytest.raises(E.EngineError):
        eng.montgomery_mul_bits_be_batch(np.zeros((1, 65), np.uint8), 513, z)
    for fmt in (1, 3):
        with pytest.raises(E.EngineError):
            eng.montgomery_to_edwards_batch(z, np.zeros(1, np.uint8), fmt)
    assert eng.montgomery_mul_batch(np.zeros((0, 32), np.uint8), np.zeros((0, 32), np.uint8)).shape == (0, 32)
    assert eng.montgomery_mul_base_batch(np.zeros((0, 32), np.uint8)).shape == (0, 32)
    out, st = eng.montgomery_to_edwards_batch(np.zeros((0, 32), np.uint8), np.zeros(0, np.uint8), 2)
    assert out.shape == (0, 160) and st.shape == (0,)
    # the context stays usable after the rejected calls
    assert _rows(eng.montgomery_mul_batch(_arr([bytes([1]) + bytes(31)]), _arr([NINE]))) == [NINE]


def test_plain_c(tmp_path):
    src = os.path.join(ROOT, "tests", "host", "montgomery_abi_smoke.c")
    exe = str(tmp_path / "montgomery_abi_smoke")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-o", exe, src, "-L" + LIBDIR, "-lc25519hip", "-Wl,-rpath," + LIBDIR,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "montgomery_abi_smoke ok" in out.stdout


CHILD_SCRIPT = r'''
import random, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import curve25519_dalek_amd as pkg
import pyref_montgomery as M
pkg.engine.select_library(%(lib)r)
e = pkg.Engine(0)
rng = random.Random(90)
ks = [rng.randbytes(32) for _ in range(600)]; us = [rng.randbytes(32) for _ in range(600)]
ks[0] = b"\xff" * 32; us[1] = b"\xff" * 32; us[2] = bytes(32)
arr = lambda xs: np.frombuffer(b"".join(xs), np.uint8).reshape(-1, 32).copy()
got = e.montgomery_mul_batch(arr(ks), arr(us))
assert all(bytes(got[i]) == M.mul(us[i], ks[i]) for i in range(600))
bits = np.frombuffer(rng.randbytes(600 * 64), np.uint8).reshape(600, 64).copy()
got = e.montgomery_mul_bits_be_batch(bits, 512, arr(us))
assert all(bytes(got[i]) == M.mul_bits_be(us[i], list(np.unpackbits(bits[i]))) for i in range(600))
e.montgomery_mul_base_batch(arr(ks))
sg = np.frombuffer(rng.randbytes(600), np.uint8).copy()
for fmt in (0, 2):
    out, st = e.montgomery_to_edwards_batch(arr(us), sg, fmt)
    assert all(int(st[i]) == (M.to_edwards(us[i], int(sg[i])) is not None) for i in range(600))
e.synchronize()
print("child montgomery ok")
'''


@pytest.mark.parametrize("which", ["debug", "per_lane_inversion"])
def test_debug_library_and_per_lane_inversion_arm(which):
    """the bound-checking debug library (no limb bound violated), and the per-lane-inversion A/B arm of to_edwards in the tuning build"""
    if which == "debug":
        lib, env = os.path.join(LIBDIR, "libc25519hip_dbg.so"), dict(os.environ)
    else:
        lib, env = util.TUNE_LIB, util.tune_env({"C25519_MONT_TO_EDWARDS_BATCHED": "0"})
    assert os.path.exists(lib), "run __graft_entry__.build()"
    code = CHILD_SCRIPT % dict(root=ROOT, lib=lib)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0 and "child montgomery ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
