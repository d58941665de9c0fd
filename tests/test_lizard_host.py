"""CPU tests of the Lizard device code (curve25519-dalek_amd/csrc/lizard.h, csrc/sha256.h), no GPU needed.

tests/host/lizard_host.cpp builds the __host__ __device__ headers for the host with C25519_CHECK_BOUNDS (a violated limb bound
aborts).  Every function is compared with hashlib, with the reference's vectors (tests/golden/lizard_vectors.json) and with the
big-integer restatement tests/pyref_lizard.py, which must reproduce the vectors and the constant identities first.
"""
import ctypes as C
import hashlib
import json
import os
import random
import subprocess

import pytest

import pyref_h2c as H
import pyref_lizard as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = L.P
VEC = json.load(open(os.path.join(ROOT, "tests", "golden", "lizard_vectors.json")))


@pytest.fixture(scope="module")
def host():
    src = os.path.join(ROOT, "tests", "host", "lizard_host.cpp")
    so = os.path.join(ROOT, "tests", "host", "liblizardhost.so")
    deps = [src] + [os.path.join(ROOT, "curve25519-dalek_amd", "csrc", f)
                    for f in ("lizard.h", "sha256.h", "h2c.h", "fe26.h", "ge26.h", "sc_sha.h", "constants_gen.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, src])
    lib = C.CDLL(so)
    for f in ("h_lizard_decode", "h_lizard_decode_compressed", "h_map_to_curve_inverse"):
        getattr(lib, f).restype = C.c_uint32
    return lib


def pt_bytes(pt):
    return b"".join((c % P).to_bytes(32, "little") for c in pt)


def decode(host, pt):
    o = C.create_string_buffer(16)
    nf = host.h_lizard_decode(pt_bytes(pt), o)
    return nf, o.raw


def decode_compressed(host, enc):
    o = C.create_string_buffer(16)
    st = host.h_lizard_decode_compressed(bytes(enc), o)
    return st, o.raw


def inverse(host, pt):
    o = C.create_string_buffer(512)
    mask = host.h_map_to_curve_inverse(pt_bytes(pt), o)
    return [o.raw[32 * j:32 * j + 32] if mask >> j & 1 else None for j in range(16)], o.raw, mask


def restricted(rng):
    b = bytearray(rng.randbytes(32))
    b[0] &= 0xFE
    b[31] &= 0x3F
    return bytes(b)


def random_point(rng):
    return H.ristretto_from_uniform_point(rng.randbytes(64))


def representatives(pt, rng):
    """the given representative, a rescaled one, and rescaled + E[4] shifts"""
    out = [pt, L.scale(pt, rng.randrange(2, P))]
    for t in L.E4[1:]:
        out.append(L.scale(H.ed_add(pt, t), rng.randrange(1, P)))
    return out


def identity_coset():
    return [L.scale(t, 1) for t in L.E4] + [L.scale(L.E4[1], 5), L.scale((0, 1, 1, 0), 7)]


# ---- the restatement against the reference's data -------------------------------------------------------------------
def test_pyref_reproduces_vectors_and_constants():
    for d, e in VEC["encode"]:
        d = bytes.fromhex(d)
        assert L.lizard_encode(d).hex() == e
        assert L.lizard_decode(L.ristretto_decode(bytes.fromhex(e))) == d
    assert len(VEC["encode"]) == 4
    for name, limbs in VEC["constants"].items():
        assert sum(x << (51 * i) for i, x in enumerate(limbs)) % P == L.CONSTANTS[name], name
    # the identities of the reference's test_lizard_constants
    assert L.SQRT_ID == L.sqrt_ratio_m1(L.SQRT_M1 * L.D, 1)[1] and L.SQRT_ID ** 2 % P == L.SQRT_M1 * L.D % P
    assert L.DP1_OVER_DM1 * (L.D - 1) % P == (L.D + 1) % P
    assert L.MDOUBLE_INVSQRT_A_MINUS_D == (-2 * H.INVSQRT_A_MINUS_D) % P
    assert L.MIDOUBLE_INVSQRT_A_MINUS_D == L.MDOUBLE_INVSQRT_A_MINUS_D * L.SQRT_M1 % P
    assert L.MINVSQRT_ONE_PLUS_D ** 2 * (1 + L.D) % P == 1 and L.is_neg(P - L.MINVSQRT_ONE_PLUS_D) == 0
    # the corner input of elligator_inv is +sqrt(i d)
    assert H.fe_from_bytes(bytes.fromhex(VEC["sqrt_id_corner"])) == L.SQRT_ID


def test_pyref_8_hash_rule_equals_16_hash_decode():
    rng = random.Random(41)
    pts = [random_point(rng) for _ in range(40)]
    pts += [L.lizard_encode_point(rng.randbytes(16)) for _ in range(40)]
    pts += [H.ristretto_map(0), H.ristretto_map(L.SQRT_ID)] + identity_coset()
    for pt in list(pts):
        pts += representatives(pt, rng)[1:]
    for pt in pts:
        assert L.lizard_decode_8(pt) == L.lizard_decode_16(pt)
    # elligator(0): both zero slots defined (slot k and 8 + k hold the same 0)
    inv = L.elligator_inverse(H.ristretto_map(0))
    zeros = [j for j in range(16) if inv[j] == 0]
    assert zeros and all(j + 8 in zeros for j in zeros if j < 8)


def test_pyref_slot_order_depends_on_the_representative_and_the_set_does_not():
    rng = random.Random(42)
    changed = 0
    for _ in range(60):
        pt = H.ristretto_map(H.fe_from_bytes(restricted(rng)))
        a, b = L.map_to_curve_inverse(pt), L.map_to_curve_inverse(L.scale(pt, rng.randrange(2, P)))
        assert sorted(x for x in a if x) == sorted(x for x in b if x)
        changed += a != b
    assert changed > 0


# ---- SHA-256 ----------------------------------------------------------------------------------------------------------
def test_sha256_16(host):
    rng = random.Random(43)
    for d in [bytes(16), b"\xff" * 16, bytes(range(16))] + [rng.randbytes(16) for _ in range(500)]:
        o = C.create_string_buffer(32)
        host.h_sha256_16(d, o)
        assert o.raw == hashlib.sha256(d).digest()


# ---- encode -----------------------------------------------------------------------------------------------------------
def test_encode_vectors(host):
    for d, e in VEC["encode"]:
        o = C.create_string_buffer(32)
        host.h_lizard_encode(bytes.fromhex(d), o)
        assert o.raw.hex() == e


def test_encode_random_vs_pyref(host):
    rng = random.Random(44)
    for _ in range(400):
        d = rng.randbytes(16)
        o = C.create_string_buffer(32)
        host.h_lizard_encode(d, o)
        assert o.raw == L.lizard_encode(d)


# ---- decode -----------------------------------------------------------------------------------------------------------
def test_decode_vectors_compressed(host):
    for d, e in VEC["encode"]:
        assert decode_compressed(host, bytes.fromhex(e)) == (1, bytes.fromhex(d))


def test_encode_then_decode_is_the_identity_on_every_representative(host):
    rng = random.Random(45)
    for _ in range(60):
        d = rng.randbytes(16)
        assert decode_compressed(host, L.lizard_encode(d)) == (1, d)
        for rep in representatives(L.lizard_encode_point(d), rng):
            assert decode(host, rep) == (1, d)


def test_random_points_decode_to_none(host):
    rng = random.Random(46)
    for _ in range(100):
        pt = random_point(rng)
        nf, pay = decode(host, pt)
        assert (nf, pay) == (L.lizard_decode_8(pt)[0], bytes(16)) and nf == 0
        assert decode_compressed(host, H.ristretto_encode(pt)) == (0, bytes(16))


def test_bad_encodings(host):
    rng = random.Random(47)
    enc = L.lizard_encode(rng.randbytes(16))
    s = int.from_bytes(enc, "little")
    for bad in ((P - s).to_bytes(32, "little"), (s + P).to_bytes(32, "little") if s + P < 2**256 else None, b"\xff" * 32, (P + 2).to_bytes(32, "little")):
        if bad is not None:
            assert L.ristretto_decode(bad) is None
            assert decode_compressed(host, bad) == (2, bytes(16))


def test_special_points(host):
    rng = random.Random(48)
    special = identity_coset() + [H.ristretto_map(0), H.ristretto_map(L.SQRT_ID)]
    special += [L.scale(p, rng.randrange(2, P)) for p in special]
    for pt in special:
        nf, pay = decode(host, pt)
        assert nf == L.lizard_decode_16(pt)[0]
        got, _, _ = inverse(host, pt)
        assert got == L.map_to_curve_inverse(pt)
    assert decode_compressed(host, bytes(32)) == (0, bytes(16))


# ---- map_to_curve_inverse ---------------------------------------------------------------------------------------------
def test_inverse_slot_order_on_the_given_coordinates(host):
    rng = random.Random(49)
    for _ in range(80):
        pt = H.ristretto_map(H.fe_from_bytes(restricted(rng)))
        for rep in representatives(pt, rng):
            got, raw, mask = inverse(host, rep)
            assert got == L.map_to_curve_inverse(rep)
            assert all(raw[32 * j:32 * j + 32] == bytes(32) for j in range(16) if not mask >> j & 1)
            assert (mask & 0xFF) == mask >> 8


def test_inverse_properties(host):
    """every defined preimage maps back; a restricted input is found in slots 0..7, exactly once"""
    rng = random.Random(50)
    for _ in range(60):
        b = restricted(rng)
        pt = H.ristretto_map(H.fe_from_bytes(b))
        enc = H.ristretto_encode(pt)
        got, _, _ = inverse(host, pt)
        assert got[:8].count(b) == 1 and b not in got[8:]
        for x in got:
            if x is not None:
                assert H.ristretto_map_to_curve(x) == enc
        for x in got[8:]:
            if x is not None and x != bytes(32):
                assert x[0] & 1
    for _ in range(40):
        b = rng.randbytes(32)
        pt = H.ristretto_map(H.fe_from_bytes(b))
        got, _, _ = inverse(host, pt)
        assert any(got)
        assert all(H.ristretto_map_to_curve(x) == H.ristretto_encode(pt) for x in got if x is not None)
