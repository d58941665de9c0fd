"""Lizard on the GPU (csrc/lizard.hip): RistrettoPoint::lizard_encode / lizard_decode::<Sha256> and map_to_curve_inverse, through
dalek.*, Engine (host twins and device tensors) and plain C, against the reference's vectors (tests/golden/lizard_vectors.json)
and the big-integer restatement tests/pyref_lizard.py."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import pyref_h2c as H
import pyref_lizard as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = json.load(open(os.path.join(ROOT, "tests", "golden", "lizard_vectors.json")))
LIBDIR = os.path.join(ROOT, "curve25519-dalek_amd", "lib")
P = L.P


@pytest.fixture(scope="module")
def eng():
    import curve25519_dalek_amd as pkg
    return pkg.Engine(0)


def _rows(a):
    return [bytes(a[i]) for i in range(a.shape[0])]


def _raw160(pt):
    """extended (X, Y, Z, T) -> RAW160: four field elements as 5 x u64 radix-2^51 limbs"""
    out = b""
    for c in pt:
        c %= P
        out += b"".join(((c >> (51 * i)) & (2**51 - 1)).to_bytes(8, "little") for i in range(5))
    return out


def _arr(items, width):
    return np.frombuffer(b"".join(items), np.uint8).reshape(-1, width).copy()


def _restricted(rng):
    b = bytearray(rng.randbytes(32))
    b[0] &= 0xFE
    b[31] &= 0x3F
    return bytes(b)


def _inverse_lists(out, mask):
    return [[bytes(out[i, j]) if int(mask[i]) >> j & 1 else None for j in range(16)] for i in range(out.shape[0])]


# ---- fixtures -------------------------------------------------------------------------------------------------------
def test_vectors_through_dalek(eng):
    from curve25519_dalek_amd import dalek
    datas = [bytes.fromhex(d) for d, _ in VEC["encode"]]
    encs = [bytes.fromhex(e) for _, e in VEC["encode"]]
    assert dalek.RistrettoPoint.lizard_encode(datas, engine=eng) == encs
    assert dalek.RistrettoPoint.lizard_decode(encs, engine=eng) == datas
    invs = dalek.RistrettoPoint.map_to_curve_inverse(encs, engine=eng)
    assert invs == [L.map_to_curve_inverse(L.ristretto_decode(e)) for e in encs]
    for d, inv in zip(datas, invs):
        assert inv[:8].count(L.tagged(d)) == 1
    # map_to_curve_restricted: the reference's panics are ValueError
    rng = random.Random(60)
    ins = [_restricted(rng) for _ in range(50)] + [bytes.fromhex(VEC["sqrt_id_corner"])]
    assert dalek.RistrettoPoint.map_to_curve_restricted(ins, engine=eng) == [H.ristretto_map_to_curve(b) for b in ins]
    for bad in (b"\x01" + bytes(31), bytes(31) + b"\x40", bytes(31) + b"\x80"):
        with pytest.raises(ValueError):
            dalek.RistrettoPoint.map_to_curve_restricted([bad], engine=eng)
    with pytest.raises(ValueError):
        dalek.RistrettoPoint.lizard_encode([bytes(15)], engine=eng)
    # invalid encodings: None
    assert dalek.RistrettoPoint.lizard_decode([b"\xff" * 32], engine=eng) == [None]
    assert dalek.RistrettoPoint.map_to_curve_inverse([b"\xff" * 32], engine=eng) == [None]


def test_vectors_through_plain_c(tmp_path):
    src = os.path.join(ROOT, "tests", "host", "lizard_abi_smoke.c")
    exe = str(tmp_path / "lizard_abi_smoke")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-o", exe, src, "-L" + LIBDIR, "-lc25519hip", "-Wl,-rpath," + LIBDIR,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "lizard_abi_smoke ok" in out.stdout


# ---- random inputs against the restatement ----------------------------------------------------------------------------
def test_encode_decode_random_vs_pyref(eng):
    rng = random.Random(61)
    datas = [rng.randbytes(16) for _ in range(2048)]
    enc = eng.ristretto_lizard_encode_batch(_arr(datas, 16))
    assert _rows(enc) == [L.lizard_encode(d) for d in datas]
    pay, st = eng.ristretto_lizard_decode_batch(enc)
    assert (st == 1).all() and _rows(pay) == datas
    raw = eng.ristretto_lizard_encode_batch(_arr(datas, 16), 2)
    assert np.array_equal(eng.compress_batch(raw, 1), enc)
    pay2, st2 = eng.ristretto_lizard_decode_batch(raw, 2)
    assert (st2 == 1).all() and np.array_equal(pay2, pay)


def test_inverse_random_vs_pyref_in_slot_order(eng):
    rng = random.Random(62)
    pts = [H.ristretto_map(H.fe_from_bytes(_restricted(rng))) for _ in range(300)]
    pts += [H.ristretto_from_uniform_point(rng.randbytes(64)) for _ in range(100)]
    encs = [H.ristretto_encode(p) for p in pts]
    out, mask, ok = eng.ristretto_map_to_curve_inverse_batch(_arr(encs, 32))
    assert ok.all()
    want = [L.map_to_curve_inverse(L.ristretto_decode(e)) for e in encs]
    assert _inverse_lists(out, mask) == want
    assert all(not out[i, j].any() for i in range(out.shape[0]) for j in range(16) if not int(mask[i]) >> j & 1)
    # RAW160 on the given coordinates, rescaled: the reference's order for that same representative
    reps = [L.scale(p, rng.randrange(2, P)) for p in pts]
    out, mask, _ = eng.ristretto_map_to_curve_inverse_batch(_arr([_raw160(p) for p in reps], 160), 2)
    assert _inverse_lists(out, mask) == [L.map_to_curve_inverse(p) for p in reps]


def test_representatives_decode_to_the_same_payload(eng):
    rng = random.Random(63)
    datas, reps = [], []
    for _ in range(200):
        d = rng.randbytes(16)
        pt = L.lizard_encode_point(d)
        for t in L.E4:
            datas.append(d)
            reps.append(L.scale(H.ed_add(pt, t), rng.randrange(1, P)))
    pay, st = eng.ristretto_lizard_decode_batch(_arr([_raw160(p) for p in reps], 160), 2)
    assert (st == 1).all() and _rows(pay) == datas


def test_bad_encodings_and_random_points(eng):
    rng = random.Random(64)
    encs = [bytes.fromhex(e) for _, e in VEC["encode"]]
    bad = []
    for e in encs:
        s = int.from_bytes(e, "little")
        bad.append((P - s).to_bytes(32, "little"))                        # negative s
        if s + P < 2**256:
            bad.append((s + P).to_bytes(32, "little"))                    # non-canonical
    bad += [b"\xff" * 32, (P + 2).to_bytes(32, "little"), bytes(31) + b"\x80"]
    assert all(L.ristretto_decode(b) is None for b in bad)
    rnd = [H.ristretto_from_uniform_bytes(rng.randbytes(64)) for _ in range(500)]
    pay, st = eng.ristretto_lizard_decode_batch(_arr(bad + rnd, 32))
    assert list(st[:len(bad)]) == [2] * len(bad)
    assert not any(L.lizard_decode(L.ristretto_decode(e)) for e in rnd[:50])
    assert (st[len(bad):] == 0).all()
    assert not pay.any()
    _, _, ok = eng.ristretto_map_to_curve_inverse_batch(_arr(bad + rnd[:10], 32))
    assert list(ok) == [0] * len(bad) + [1] * 10


def test_special_points(eng):
    special = [(0, 1, 1, 0), L.E4[1], L.E4[2], L.E4[3], H.ristretto_map(0), H.ristretto_map(L.SQRT_ID), L.scale(L.E4[1], 9)]
    pay, st = eng.ristretto_lizard_decode_batch(_arr([_raw160(p) for p in special], 160), 2)
    assert list(st) == [0] * len(special) and not pay.any()
    out, mask, _ = eng.ristretto_map_to_curve_inverse_batch(_arr([_raw160(p) for p in special], 160), 2)
    assert _inverse_lists(out, mask) == [L.map_to_curve_inverse(p) for p in special]
    pay, st = eng.ristretto_lizard_decode_batch(np.zeros((1, 32), np.uint8))
    assert list(st) == [0]


# ---- sizes, device tensors, statuses ----------------------------------------------------------------------------------
def test_sizes_and_device_tensors(eng):
    import torch
    rng = random.Random(65)
    for n in (0, 1, 255, 257, 1000):
        d = np.frombuffer(rng.randbytes(n * 16), np.uint8).reshape(-1, 16).copy()
        enc = eng.ristretto_lizard_encode_batch(d)
        assert enc.shape == (n, 32)
        td = torch.from_numpy(d).to(eng.device)
        tenc = eng.ristretto_lizard_encode_batch_t(td)
        assert np.array_equal(tenc.cpu().numpy(), enc)
        traw = eng.ristretto_lizard_encode_batch_t(td, 2)
        for t, fmt in ((tenc, 1), (traw, 2)):
            pay, st = eng.ristretto_lizard_decode_batch_t(t, fmt)
            assert np.array_equal(pay.cpu().numpy(), d) and (st.cpu().numpy() == 1).all()
            out, mask, ok = eng.ristretto_map_to_curve_inverse_batch_t(t, fmt)
            hout, hmask, hok = eng.ristretto_map_to_curve_inverse_batch(t.cpu().numpy(), fmt)
            assert np.array_equal(out.cpu().numpy(), hout) and np.array_equal(mask.cpu().numpy().view(np.uint16), hmask)
            assert (ok.cpu().numpy() == 1).all() and (hok == 1).all()


def test_large_round_trip(eng):
    n = 1 << 18
    rng = np.random.default_rng(66)
    d = rng.integers(0, 256, size=(n, 16), dtype=np.uint8)
    enc = eng.ristretto_lizard_encode_batch(d)
    raw = eng.ristretto_lizard_encode_batch(d, 2)
    for a, fmt in ((enc, 1), (raw, 2)):
        pay, st = eng.ristretto_lizard_decode_batch(a, fmt)
        assert (st == 1).all() and np.array_equal(pay, d)
    for i in list(range(0, 32)) + list(rng.integers(0, n, 128)) + list(range(n - 32, n)):
        assert bytes(enc[i]) == L.lizard_encode(bytes(d[i])), i


def test_bad_formats_and_empty(eng):
    import curve25519_dalek_amd as pkg
    E = pkg.engine
    z = np.zeros((1, 32), np.uint8)
    with pytest.raises(E.EngineError):
        eng.ristretto_lizard_encode_batch(np.zeros((1, 16), np.uint8), out_fmt=0)
    with pytest.raises(E.EngineError):
        eng.ristretto_lizard_decode_batch(z, in_fmt=0)
    with pytest.raises(E.EngineError):
        eng.ristretto_map_to_curve_inverse_batch(z, in_fmt=0)
    assert eng.ristretto_lizard_encode_batch(np.zeros((0, 16), np.uint8)).shape == (0, 32)
    pay, st = eng.ristretto_lizard_decode_batch(np.zeros((0, 32), np.uint8))
    assert pay.shape == (0, 16) and st.shape == (0,)
    out, mask, ok = eng.ristretto_map_to_curve_inverse_batch(np.zeros((0, 160), np.uint8), 2)
    assert out.shape == (0, 16, 32)
    # the context stays usable after the rejected calls
    d = bytes.fromhex(VEC["encode"][2][0])
    assert _rows(eng.ristretto_lizard_encode_batch(np.frombuffer(d, np.uint8).reshape(1, 16))) == [bytes.fromhex(VEC["encode"][2][1])]


# ---- the bound-checking debug library ---------------------------------------------------------------------------------
DEBUG_SCRIPT = r'''
import random, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import curve25519_dalek_amd as pkg
import pyref_h2c as H, pyref_lizard as L
pkg.engine.select_library(%(lib)r)
e = pkg.Engine(0)
rng = random.Random(71)
d = np.frombuffer(rng.randbytes(3000 * 16), np.uint8).reshape(-1, 16).copy(); d[0] = 0; d[1] = 0xFF
enc = e.ristretto_lizard_encode_batch(d)
assert all(bytes(enc[i]) == L.lizard_encode(bytes(d[i])) for i in range(0, 3000, 7))
raw = e.ristretto_lizard_encode_batch(d, 2)
for a, f in ((enc, 1), (raw, 2)):
    pay, st = e.ristretto_lizard_decode_batch(a, f)
    assert (st == 1).all() and np.array_equal(pay, d)
    out, mask, ok = e.ristretto_map_to_curve_inverse_batch(a, f)
rnd = np.frombuffer(b"".join(H.ristretto_from_uniform_bytes(rng.randbytes(64)) for _ in range(300)) + b"\xff" * 32 + bytes(32), np.uint8).reshape(-1, 32).copy()
pay, st = e.ristretto_lizard_decode_batch(rnd)
assert list(st[-2:]) == [2, 0] and (st[:300] == 0).all()
e.ristretto_map_to_curve_inverse_batch(rnd)
e.synchronize()
print("debug lizard ok")
'''


def test_debug_library_runs_without_a_bound_assert():
    lib = os.path.join(LIBDIR, "libc25519hip_dbg.so")
    assert os.path.exists(lib), "run __graft_entry__.build() (make debug)"
    code = DEBUG_SCRIPT % dict(root=ROOT, lib=lib)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "debug lizard ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
