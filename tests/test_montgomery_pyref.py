"""The big-integer MontgomeryPoint restatement (tests/pyref_montgomery.py) against the reference's own montgomery.rs cases
(tests/golden/montgomery_vectors.json) and against the independent RFC 7748 ladder and Edwards arithmetic of tests/pyref.py.
CPU only: this is the yardstick tests/test_gpu_montgomery.py holds the kernels to."""
import hashlib
import json
import os
import random

import pyref as R
import pyref_montgomery as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = json.load(open(os.path.join(ROOT, "tests", "golden", "montgomery_vectors.json")))
P = M.P


def test_basepoint_and_twist_cases_of_the_reference():
    for u, sign, want in VEC["to_edwards"]:
        got = M.to_edwards(bytes.fromhex(u), sign)
        assert got == (bytes.fromhex(want) if want is not None else None), (u, sign)
    # basepoint_edwards_to_montgomery
    assert M.to_montgomery(R.B) == bytes.fromhex(VEC["x25519_basepoint"])
    assert R.ed_compress(R.B) == bytes.fromhex(VEC["ed25519_basepoint"])


def test_eq_defined_mod_p():
    a, b = (bytes.fromhex(x) for x in VEC["eq_defined_mod_p"])
    assert M.from_bytes(a) == M.from_bytes(b) == 18
    k = hashlib.sha256(b"k").digest()
    assert M.mul(a, k) == M.mul(b, k)
    assert M.to_edwards(a, 0) == M.to_edwards(b, 0) and M.to_edwards(a, 1) == M.to_edwards(b, 1)


def test_ladder_matches_edwards_scalarmult():
    for u, s, want in VEC["ladder_matches_edwards"]:
        assert M.mul(bytes.fromhex(u), bytes.fromhex(s)) == bytes.fromhex(want)


def test_mul_of_a_clamped_scalar_is_x25519():
    rng = random.Random(5)
    for _ in range(20):
        k, u = rng.randbytes(32), rng.randbytes(32)
        kb = bytearray(k); kb[0] &= 248; kb[31] &= 127; kb[31] |= 64
        assert M.mul(u, bytes(kb)) == R.x25519(k, u)


def test_mul_skips_bit_255_and_mul_bits_be_agrees():
    rng = random.Random(6)
    for _ in range(10):
        k, u = bytearray(rng.randbytes(32)), rng.randbytes(32)
        k[31] &= 0x7F
        k1 = bytes(k); k[31] |= 0x80
        assert M.mul(u, bytes(k)) == M.mul(u, k1) == M.mul_bits_be(u, M.scalar_bits_be(k1, 255))
    # leading zero bits change nothing; the empty string is the identity
    u = rng.randbytes(32)
    assert M.mul_bits_be(u, [0] * 40 + [1, 0, 1]) == M.mul_bits_be(u, [1, 0, 1])
    assert M.mul_bits_be(u, []) == bytes(32)


def test_mul_bits_be_is_an_integer_multiple_on_the_prime_order_subgroup():
    # montgomery.rs montgomery_mul_bits_be: a 512-bit integer b, b P on the Montgomery side = (b mod l) P on the Edwards side
    rng = random.Random(7)
    for _ in range(3):
        pe = R.ed_mul(rng.randrange(R.L), R.B)
        b = rng.getrandbits(512)
        bits = [(b >> i) & 1 for i in reversed(range(512))]
        assert M.mul_bits_be(M.to_montgomery(pe), bits) == M.to_montgomery(R.ed_mul(b % R.L, pe))


def test_mul_base_and_to_edwards_round_trip():
    rng = random.Random(8)
    for _ in range(10):
        s = rng.randrange(R.L).to_bytes(32, "little")
        pe = R.ed_mul(int.from_bytes(s, "little"), R.B)
        assert M.mul_base(s) == M.mul(bytes.fromhex(VEC["x25519_basepoint"]), s) == M.to_montgomery(pe)
        assert M.to_edwards_point(M.mul_base(s), pe[0] & 1) == pe
    # u = 0: y = -1, x = 0 -- with sign 1 the decoded x stays 0 ("negative zero") and the encoding is y alone
    assert M.to_edwards_point(bytes(32), 1) == (0, P - 1)
    assert M.to_edwards(bytes(32), 1) == M.to_edwards(bytes(32), 0) == (P - 1).to_bytes(32, "little")
    # only bit 0 of the u8 sign counts
    u = bytes.fromhex(VEC["x25519_basepoint"])
    assert M.to_edwards(u, 2) == M.to_edwards(u, 0) and M.to_edwards(u, 3) == M.to_edwards(u, 1)
