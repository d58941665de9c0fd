"""Hash-to-group on the GPU (csrc/h2c.hip): Ristretto from_uniform_bytes / map_to_curve / hash_from_bytes and RFC 9380 Edwards
hash_to_curve / encode_to_curve, through dalek.*, Engine (host twins and device tensors) and plain C, against the RFC fixtures
(tests/golden/h2c_vectors.json) and the big-integer restatement tests/pyref_h2c.py."""
import hashlib
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import pyref_h2c as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = json.load(open(os.path.join(ROOT, "tests", "golden", "h2c_vectors.json")))
DST_RO = VEC["hash_to_curve"]["dst"].encode()
DST_NU = VEC["encode_to_curve"]["dst"].encode()
LIBDIR = os.path.join(ROOT, "curve25519-dalek_amd", "lib")


@pytest.fixture(scope="module")
def eng():
    import curve25519_dalek_amd as pkg
    return pkg.Engine(0)


def _edwards_enc(x, y):
    return (y | (x & 1) << 255).to_bytes(32, "little")


def _rows(a):
    return [bytes(a[i]) for i in range(a.shape[0])]


# ---- fixtures -------------------------------------------------------------------------------------------------------
def test_fixtures_through_dalek(eng):
    from curve25519_dalek_amd import dalek
    ins = [bytes.fromhex(a) for a, _ in VEC["elligator_sage"]]
    assert dalek.RistrettoPoint.map_to_curve(ins, engine=eng) == [bytes.fromhex(b) for _, b in VEC["elligator_sage"]]
    ins = [bytes.fromhex(a) for a, _ in VEC["one_way_map"]]
    assert dalek.RistrettoPoint.from_uniform_bytes(ins, engine=eng) == [bytes.fromhex(b) for _, b in VEC["one_way_map"]]
    for key, fn in (("hash_to_curve", dalek.EdwardsPoint.hash_to_curve), ("encode_to_curve", dalek.EdwardsPoint.encode_to_curve)):
        dst = VEC[key]["dst"].encode()
        msgs = [bytes.fromhex(m) for m, _, _ in VEC[key]["vectors"]]
        want = [_edwards_enc(int(x, 16), int(y, 16)) for _, x, y in VEC[key]["vectors"]]
        assert fn(msgs, dst, engine=eng) == want
        # messages and DST as pieces, as the reference's &[&[u8]]
        pieces = [[m[:1], m[1:5], m[5:]] for m in msgs]
        assert fn(pieces, [dst[:10], b"", dst[10:]], engine=eng) == want
    msgs = [b"", b"abc", b"x" * 300]
    assert dalek.RistrettoPoint.hash_from_bytes(msgs, engine=eng) == [R.ristretto_hash_from_bytes(m) for m in msgs]


def test_fixtures_through_plain_c(tmp_path):
    src = os.path.join(ROOT, "tests", "host", "h2c_abi_smoke.c")
    exe = str(tmp_path / "h2c_abi_smoke")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-o", exe, src, "-L" + LIBDIR, "-lc25519hip", "-Wl,-rpath," + LIBDIR,
                           "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert "h2c_abi_smoke ok" in out.stdout


# ---- random inputs against the restatement ----------------------------------------------------------------------------
def test_random_ristretto_vs_pyref(eng):
    rng = random.Random(21)
    a32 = np.frombuffer(rng.randbytes(4096 * 32), np.uint8).reshape(-1, 32).copy()
    a32[:4] = 0xFF; a32[4] = 0                                                      # bit 255 set, >= p, r0 = 0
    assert _rows(eng.ristretto_map_to_curve_batch(a32)) == [R.ristretto_map_to_curve(bytes(r)) for r in a32]
    a64 = np.frombuffer(rng.randbytes(4096 * 64), np.uint8).reshape(-1, 64)
    assert _rows(eng.ristretto_from_uniform_bytes_batch(a64)) == [R.ristretto_from_uniform_bytes(bytes(r)) for r in a64]
    msgs = [rng.randbytes(rng.randrange(0, 300)) for _ in range(4096)]
    assert _rows(eng.ristretto_hash_from_bytes_batch(msgs)) == [R.ristretto_hash_from_bytes(m) for m in msgs]


@pytest.mark.parametrize("mode", [1, 0], ids=["RO", "NU"])
def test_random_edwards_vs_pyref(eng, mode):
    rng = random.Random(22 + mode)
    msgs = [rng.randbytes(rng.randrange(0, 300)) for _ in range(4096)]
    dst = DST_RO if mode else DST_NU
    f = R.edwards_hash_to_curve if mode else R.edwards_encode_to_curve
    want = [f(m, dst) for m in msgs]
    assert _rows(eng.edwards_hash_to_curve_batch(msgs, dst, mode)) == [R.edwards_compress(p) for p in want]
    raw = eng.edwards_hash_to_curve_batch(msgs[:512], dst, mode, out_fmt=2)
    assert _rows(eng.compress_batch(raw, 0)) == [R.edwards_compress(p) for p in want[:512]]
    for dl in (1, 255):
        d = bytes(rng.randrange(256) for _ in range(dl))
        assert _rows(eng.edwards_hash_to_curve_batch(msgs[:300], d, mode)) == [R.edwards_compress(f(m, d)) for m in msgs[:300]]


# ---- RAW160 output feeds the rest of the engine -----------------------------------------------------------------------
def test_raw160_compresses_and_feeds_msm(eng):
    rng = random.Random(23)
    a64 = np.frombuffer(rng.randbytes(1000 * 64), np.uint8).reshape(-1, 64)
    enc = eng.ristretto_from_uniform_bytes_batch(a64, 1)
    raw = eng.ristretto_from_uniform_bytes_batch(a64, 2)
    assert np.array_equal(eng.compress_batch(raw, 1), enc)
    s = np.frombuffer(rng.randbytes(1000 * 32), np.uint8).reshape(-1, 32).copy(); s[:, 31] &= 0x0F
    st1, r1 = eng.msm_vartime(s, raw, in_fmt=2, out_fmt=1)
    st2, r2 = eng.msm_vartime(s, enc, in_fmt=1, out_fmt=1)
    assert st1 == 0 and st2 == 0 and r1 == r2
    a32 = a64[:, :32].copy()
    assert np.array_equal(eng.compress_batch(eng.ristretto_map_to_curve_batch(a32, 2), 1), eng.ristretto_map_to_curve_batch(a32, 1))


def test_from_uniform_is_sum_of_two_maps(eng):
    """from_uniform_bytes(a || b) == map(a) + map(b), the sum taken by a 2-term MSM with unit scalars over the RAW160 maps"""
    rng = random.Random(24)
    one = np.zeros((2, 32), np.uint8); one[:, 0] = 1
    for _ in range(16):
        a, b = rng.randbytes(32), rng.randbytes(32)
        pts = eng.ristretto_map_to_curve_batch(np.frombuffer(a + b, np.uint8).reshape(2, 32), 2)
        st, r = eng.msm_vartime(one, pts, in_fmt=2, out_fmt=1)
        assert st == 0 and r == bytes(eng.ristretto_from_uniform_bytes_batch(np.frombuffer(a + b, np.uint8).reshape(1, 64))[0])


def test_hash_from_bytes_is_from_uniform_of_sha512(eng):
    rng = random.Random(25)
    msgs = [rng.randbytes(rng.randrange(0, 200)) for _ in range(700)]
    dig = np.frombuffer(b"".join(hashlib.sha512(m).digest() for m in msgs), np.uint8).reshape(-1, 64)
    assert np.array_equal(eng.ristretto_hash_from_bytes_batch(msgs), eng.ristretto_from_uniform_bytes_batch(dig))
    assert np.array_equal(eng.ristretto_hash_from_bytes_batch(msgs, 2)[:5].shape, (5, 160))


# ---- sizes, device tensors, statuses ----------------------------------------------------------------------------------
def test_sizes_and_device_tensors(eng):
    import torch
    rng = random.Random(26)
    for n in (0, 1, 255, 257, 1000):
        a64 = np.frombuffer(rng.randbytes(n * 64), np.uint8).reshape(-1, 64)
        got = eng.ristretto_from_uniform_bytes_batch(a64)
        assert got.shape == (n, 32) and _rows(got) == [R.ristretto_from_uniform_bytes(bytes(r)) for r in a64]
        t = torch.from_numpy(a64.copy()).to(eng.device)
        assert np.array_equal(eng.ristretto_from_uniform_bytes_batch_t(t).cpu().numpy(), got)
        assert np.array_equal(eng.ristretto_map_to_curve_batch_t(t.view(-1, 32)[: n].contiguous()).cpu().numpy(),
                              eng.ristretto_map_to_curve_batch(a64.reshape(-1, 32)[:n].copy()))
        msgs = [rng.randbytes(rng.randrange(0, 130)) for _ in range(n)]
        blob, off = eng._pack(msgs)
        tb, to = torch.from_numpy(blob.copy()).to(eng.device), torch.from_numpy(off.astype(np.int64)).to(eng.device)
        assert np.array_equal(eng.ristretto_hash_from_bytes_batch_t(tb, to).cpu().numpy(), eng.ristretto_hash_from_bytes_batch(msgs))
        assert np.array_equal(eng.edwards_hash_to_curve_batch_t(tb, to, DST_RO).cpu().numpy(), eng.edwards_hash_to_curve_batch(msgs, DST_RO))


def test_large_call(eng):
    n = 1 << 18
    rng = np.random.default_rng(27)
    a64 = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
    got = eng.ristretto_from_uniform_bytes_batch(a64)
    for i in list(range(0, 64)) + list(rng.integers(0, n, 256)) + list(range(n - 64, n)):
        assert bytes(got[i]) == R.ristretto_from_uniform_bytes(bytes(a64[i])), i


def test_bad_dst_and_offsets(eng):
    import torch
    import curve25519_dalek_amd as pkg
    from curve25519_dalek_amd import dalek
    E = pkg.engine
    for bad in (b"", b"x" * 256):
        assert eng.edwards_hash_to_curve_batch([b"abc"], bad) == E.DOMAIN_SEPARATOR_LENGTH
        with pytest.raises(dalek.DomainSeparatorError):
            dalek.EdwardsPoint.hash_to_curve([b"abc"], bad, engine=eng)
    assert eng.edwards_hash_to_curve_batch([b"a" * 10], b"x" * 255).shape == (1, 32)
    blob = torch.zeros(16, dtype=torch.uint8, device=eng.device)
    for off in ([0, 5, 3], [0, 3, 17]):                 # not monotone; past msgs_len
        to = torch.tensor(off, dtype=torch.int64, device=eng.device)
        with pytest.raises(E.EngineError, match="msg_off"):
            eng.ristretto_hash_from_bytes_batch_t(blob, to)
        with pytest.raises(E.EngineError, match="msg_off"):
            eng.edwards_hash_to_curve_batch_t(blob, to, DST_RO)
    with pytest.raises(E.EngineError):
        eng.ristretto_hash_from_bytes_batch(b"abc", msg_off=np.array([0, 3, 1], np.uint64))
    with pytest.raises(E.EngineError):
        eng.ristretto_map_to_curve_batch(np.zeros((1, 32), np.uint8), out_fmt=0)
    with pytest.raises(E.EngineError):
        eng.edwards_hash_to_curve_batch([b"a"], DST_RO, out_fmt=1)
    # the context stays usable after the rejected calls
    assert _rows(eng.edwards_hash_to_curve_batch([b"abc"], DST_RO)) == [R.edwards_compress(R.edwards_hash_to_curve(b"abc", DST_RO))]


# ---- the bound-checking debug library ---------------------------------------------------------------------------------
DEBUG_SCRIPT = r'''
import random, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import curve25519_dalek_amd as pkg
import pyref_h2c as R
pkg.engine.select_library(%(lib)r)
e = pkg.Engine(0)
rng = random.Random(31)
a64 = np.frombuffer(rng.randbytes(3000 * 64), np.uint8).reshape(-1, 64).copy(); a64[:3] = 0xFF; a64[3] = 0
got = e.ristretto_from_uniform_bytes_batch(a64)
assert all(bytes(got[i]) == R.ristretto_from_uniform_bytes(bytes(a64[i])) for i in range(0, 3000, 7))
raw = e.ristretto_from_uniform_bytes_batch(a64, 2)
assert np.array_equal(e.compress_batch(raw, 1), got)
m32 = e.ristretto_map_to_curve_batch(a64[:, :32].copy())
assert all(bytes(m32[i]) == R.ristretto_map_to_curve(bytes(a64[i, :32])) for i in range(0, 3000, 7))
msgs = [rng.randbytes(rng.randrange(0, 300)) for _ in range(2000)] + [b""]
h = e.ristretto_hash_from_bytes_batch(msgs)
assert all(bytes(h[i]) == R.ristretto_hash_from_bytes(msgs[i]) for i in range(0, 2001, 11))
for mode, dst, f in ((1, %(ro)r, R.edwards_hash_to_curve), (0, %(nu)r, R.edwards_encode_to_curve)):
    for d in (dst, b"z", b"y" * 255):
        out = e.edwards_hash_to_curve_batch(msgs, d, mode)
        assert all(bytes(out[i]) == R.edwards_compress(f(msgs[i], d)) for i in range(0, 2001, 13))
        e.edwards_hash_to_curve_batch(msgs, d, mode, out_fmt=2)
e.synchronize()
print("debug h2c ok")
'''


def test_debug_library_runs_without_a_bound_assert():
    lib = os.path.join(LIBDIR, "libc25519hip_dbg.so")
    assert os.path.exists(lib), "run __graft_entry__.build() (make debug)"
    code = DEBUG_SCRIPT % dict(root=ROOT, lib=lib, ro=DST_RO, nu=DST_NU)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "debug h2c ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
