"""CPU tests of the hash-to-group device code (curve25519-dalek_amd/csrc/h2c.h), no GPU needed.

tests/host/h2c_host.cpp builds the __host__ __device__ header for the host with C25519_CHECK_BOUNDS (a violated limb bound
aborts), and every function is compared with the RFC fixtures (tests/golden/h2c_vectors.json) and with the independent
big-integer restatement tests/pyref_h2c.py -- which itself must reproduce every fixture first.
"""
import ctypes as C
import hashlib
import json
import os
import random
import subprocess

import pytest

import pyref_h2c as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = R.P
VEC = json.load(open(os.path.join(ROOT, "tests", "golden", "h2c_vectors.json")))


@pytest.fixture(scope="module")
def host():
    src = os.path.join(ROOT, "tests", "host", "h2c_host.cpp")
    so = os.path.join(ROOT, "tests", "host", "libh2chost.so")
    deps = [src] + [os.path.join(ROOT, "curve25519-dalek_amd", "csrc", f) for f in ("h2c.h", "fe26.h", "ge26.h", "sc_sha.h", "constants_gen.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, src])
    return C.CDLL(so)


def call(host, name, *args, out=32):
    o = C.create_string_buffer(out)
    getattr(host, name)(*args, o)
    return o.raw


def b2i(b):
    return int.from_bytes(b, "little")


def h2c(host, msg, dst, ro):
    """-> (affine x, affine y, compressed Edwards y)"""
    o = call(host, "h_ed_hash_to_curve", msg, C.c_uint64(len(msg)), dst, C.c_uint32(len(dst)), 1 if ro else 0, out=96)
    return b2i(o[:32]), b2i(o[32:64]), o[64:]


def xmd(host, msg, dst, count):
    return call(host, "h_xmd", msg, C.c_uint64(len(msg)), dst, C.c_uint32(len(dst)), count, out=48 * count)


def h2f(host, msg, dst, count):
    o = call(host, "h_hash_to_field", msg, C.c_uint64(len(msg)), dst, C.c_uint32(len(dst)), count, out=64)
    return [b2i(o[32 * i:32 * i + 32]) for i in range(count)]


# ---- the restatement against the fixtures ---------------------------------------------------------------------------
def test_pyref_reproduces_every_fixture():
    for a, b in VEC["elligator_sage"]:
        assert R.ristretto_map_to_curve(bytes.fromhex(a)).hex() == b
    for a, b in VEC["one_way_map"]:
        assert R.ristretto_from_uniform_bytes(bytes.fromhex(a)).hex() == b
    for key, fn in (("hash_to_curve", R.edwards_hash_to_curve), ("encode_to_curve", R.edwards_encode_to_curve)):
        dst = VEC[key]["dst"].encode()
        for m, x, y in VEC[key]["vectors"]:
            assert R.affine(fn(bytes.fromhex(m), dst)) == (int(x, 16), int(y, 16))
    for key, count in (("hash_to_field_1", 1), ("hash_to_field_2", 2)):
        dst = VEC[key]["dst"].encode()
        for v in VEC[key]["vectors"]:
            assert R.hash_to_field(bytes.fromhex(v[0]), dst, count) == [int(h, 16) for h in v[1:]]
    assert len(VEC["elligator_sage"]) == 16


# ---- Ristretto map --------------------------------------------------------------------------------------------------
def test_ristretto_map_sage_vectors(host):
    for a, b in VEC["elligator_sage"]:
        assert call(host, "h_ris_map", bytes.fromhex(a)).hex() == b


def test_ristretto_one_way_map_vectors(host):
    for a, b in VEC["one_way_map"]:
        assert call(host, "h_ris_from_uniform", bytes.fromhex(a)).hex() == b


def test_ristretto_map_edge_inputs(host):
    """bit 255 masked (map(x | 2^255) == map(x)), inputs >= p reduced (map(p + k) == map(k)), r0 = 0, p - 1, 2^255 - 1"""
    rng = random.Random(11)
    edge = [0, 1, 2, 18, 19, P - 1, P, P + 1, P + 18, 2**255 - 1] + [rng.getrandbits(255) for _ in range(40)]
    for v in edge:
        b = v.to_bytes(32, "little")
        got = call(host, "h_ris_map", b)
        assert got == R.ristretto_map_to_curve(b), v
        assert call(host, "h_ris_map", (v | 1 << 255).to_bytes(32, "little")) == got
        if v < 2**255 - P:
            assert call(host, "h_ris_map", (v + P).to_bytes(32, "little")) == got
    assert call(host, "h_ris_map", bytes(32)) == bytes(32)       # r0 = 0 maps to the identity


def test_ristretto_random_vs_pyref(host):
    rng = random.Random(12)
    for _ in range(1500):
        b = rng.randbytes(32)
        assert call(host, "h_ris_map", b) == R.ristretto_map_to_curve(b)
    for _ in range(1500):
        b = rng.randbytes(64)
        assert call(host, "h_ris_from_uniform", b) == R.ristretto_from_uniform_bytes(b)


# ---- Elligator 2 and the Edwards map ---------------------------------------------------------------------------------
def test_elligator2_exceptional_case_u_zero(host):
    """u = 0: -J is a non-square, so x2 = 0 and the Montgomery point is (0, 0); the birational map's e = (xd yd == 0) fires -> identity"""
    assert not R.is_square(-486662)
    o = call(host, "h_mont_elligator2", bytes(32), out=96)
    xn, xd, y = b2i(o[:32]), b2i(o[32:64]), b2i(o[64:])
    assert xn * pow(xd, P - 2, P) % P == 0 and y == 0
    assert R.elligator2_curve25519(0) == (0, 0)
    o = call(host, "h_ed_map", bytes(32), out=64)
    assert (b2i(o[:32]), b2i(o[32:])) == (0, 1)
    for v in (P, 2 * P):         # representatives of 0 (bit 255 is masked by the loader; 2p has bit 255 clear)
        if v < 2**255:
            o = call(host, "h_ed_map", v.to_bytes(32, "little"), out=64)
            assert (b2i(o[:32]), b2i(o[32:])) == (0, 1)


def test_elligator2_and_edwards_map_random(host):
    rng = random.Random(13)
    for u in [1, 2, P - 1, (P - 1) // 2] + [rng.randrange(P) for _ in range(1500)]:
        ub = u.to_bytes(32, "little")
        o = call(host, "h_mont_elligator2", ub, out=96)
        xn, xd, y = b2i(o[:32]), b2i(o[32:64]), b2i(o[64:])
        assert (xn * pow(xd, P - 2, P) % P, y) == R.elligator2_curve25519(u)
        o = call(host, "h_ed_map", ub, out=64)
        assert (b2i(o[:32]), b2i(o[32:])) == R.affine(R.map_to_edwards25519(u))


# ---- expand_message_xmd / hash_to_field -----------------------------------------------------------------------------
def test_hash_to_field_fixtures(host):
    for key, count in (("hash_to_field_1", 1), ("hash_to_field_2", 2)):
        dst = VEC[key]["dst"].encode()
        for v in VEC[key]["vectors"]:
            assert h2f(host, bytes.fromhex(v[0]), dst, count) == [int(h, 16) for h in v[1:]]


def test_expand_message_xmd_lengths(host):
    """messages of 0 .. 300 bytes cross every SHA-512 block boundary of b_0 (128-byte Z_pad first); DST lengths 1 .. 255"""
    rng = random.Random(14)
    for n in list(range(0, 301)):
        msg = rng.randbytes(n)
        dst = rng.randbytes(rng.choice([1, 2, 7, 8, 9, 43, 64, 100, 127, 128, 200, 255]))
        for count in (1, 2):
            assert xmd(host, msg, dst, count) == R.expand_message_xmd(msg, dst, 48 * count), (n, len(dst), count)
    for dl in (1, 255):
        dst = bytes(rng.randrange(256) for _ in range(dl))
        for n in (0, 1, 63, 64, 111, 112, 127, 128, 129, 255, 256):
            msg = rng.randbytes(n)
            assert h2f(host, msg, dst, 2) == R.hash_to_field(msg, dst, 2)


def test_from_be48_reduction(host):
    rng = random.Random(15)
    for v in [0, 1, P - 1, P, 2**255 - 1, 2**255, 2**256 - 1, 2**384 - 1, 38 * 2**256] + [rng.getrandbits(384) for _ in range(500)]:
        assert b2i(call(host, "h_fe_from_be48", v.to_bytes(48, "big"))) == v % P


# ---- Edwards hash_to_curve / encode_to_curve ------------------------------------------------------------------------
def test_edwards_rfc9380_vectors(host):
    for key, ro in (("hash_to_curve", True), ("encode_to_curve", False)):
        dst = VEC[key]["dst"].encode()
        for m, x, y in VEC[key]["vectors"]:
            gx, gy, enc = h2c(host, bytes.fromhex(m), dst, ro)
            assert (gx, gy) == (int(x, 16), int(y, 16))
            assert enc == (int(y, 16) | (int(x, 16) & 1) << 255).to_bytes(32, "little")


def test_edwards_random_vs_pyref(host):
    rng = random.Random(16)
    for i in range(600):
        msg = rng.randbytes(rng.randrange(0, 300))
        dst = rng.randbytes(rng.choice([1, 16, 43, 255]))
        ro = bool(i & 1)
        want = (R.edwards_hash_to_curve if ro else R.edwards_encode_to_curve)(msg, dst)
        gx, gy, enc = h2c(host, msg, dst, ro)
        assert (gx, gy) == R.affine(want) and enc == R.edwards_compress(want)


def test_hash_from_bytes_is_from_uniform_of_sha512(host):
    rng = random.Random(17)
    for _ in range(50):
        m = rng.randbytes(rng.randrange(200))
        assert call(host, "h_ris_from_uniform", hashlib.sha512(m).digest()) == R.ristretto_hash_from_bytes(m)
