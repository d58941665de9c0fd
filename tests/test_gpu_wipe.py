"""Secrets do not stay behind: what a secret-taking entry point leaves in the context's device workspaces.

For every case, on a FRESH Engine (default flags: constant-time tables): run the call once (workspaces get allocated -- fresh device memory is not zero,
nothing is judged yet), zero every workspace (c25519_debug_workspace_zero), run the same call again with the same sizes and DIFFERENT secrets, check its
result against the oracle / hashlib / Python integers (the call demonstrably did its work), then read every workspace of the context and its peer back
(c25519_debug_workspace_read drains every stream first) and assert
  * needles: no 8-byte window of any of the call's secrets occurs anywhere (at 4-byte alignment, where every staging array and record starts): seeds, the
    expanded key a = clamp(SHA-512(seed)[:32]), the prefix, the nonce r = SHA-512(prefix || M) mod l, scalars and their clamped forms, the bit strings of
    mul_bits_be, inverses, shared secrets and other products, payloads, uniform bytes;
  * zero elsewhere: every byte of every workspace is zero outside the case's allow-list of PUBLIC leftovers, which is kept by buffer and content
    (the bytes found there must equal public values the test computes), never by offset.
Sizes: every case at a few thousand items; the cases that end in the Edwards compressor also at 4095 / 4097 (its 4096-point switch); every host form
that goes through ffi_twin also one item below and one above the size at which it starts to run in two chunks (ffi_chunk_units: twice its minimum chunk,
2^17, 2^18 or 2^19), and x25519_batch above 2^19, where its chunks are tapered.  Large cases check the result on a sample that includes both sides of
the chunk boundary.
The same after an argument error detected late (sign_batch_t with non-monotone offsets: the flag is read back after the secrets were expanded).

Not covered: the double-base and verification calls (their scalars are public by contract: vartime_double_scalar_mul_basepoint), the early returns after a
failed launch (covered by construction: the stream_wipe is in scope before the first launch), and -- a limit of any such test -- registers, LDS and caches.
A context created with FLAG_VARTIME_TABLES declares its scalars public: one case asserts equal results only, no wipe claim."""
import hashlib

import numpy as np
import pytest
import torch

import curve25519_dalek_amd as pkg
from curve25519_dalek_amd import engine as E
from oracle import orc
from util import L, rand_bytes, rand_scalars

pytestmark = pytest.mark.gpu
# a few thousand items; 4095 / 4097 straddle the 4096-point switch of the Edwards compressor (capi.hip c25519_compress_batch_dev)
SIZES = [3000, 4095, 4097]


def _clamp(raw):
    c = raw.copy()
    c[:, 0] &= 248; c[:, 31] &= 127; c[:, 31] |= 64
    return c


def _expand(seeds):
    """-> (a = clamp(h[:32]), prefix = h[32:]) rows, h = SHA-512(seed)"""
    h = np.frombuffer(b"".join(hashlib.sha512(s.tobytes()).digest() for s in seeds), dtype=np.uint8).reshape(-1, 64)
    return _clamp(h[:, :32]), h[:, 32:].copy()


def _nonces(prefix, msgs, dom=b""):
    r = [int.from_bytes(hashlib.sha512(dom + p.tobytes() + m).digest(), "little") % L for p, m in zip(prefix, msgs)]
    return np.frombuffer(b"".join(x.to_bytes(32, "little") for x in r), dtype=np.uint8).reshape(-1, 32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _keys(buf):
    """the 8-byte windows of a buffer at every 4-byte step, as uint64"""
    w = np.ascontiguousarray(buf[:len(buf) // 4 * 4]).view("<u4").astype(np.uint64)
    return w[:-1] | (w[1:] << np.uint64(32)) if len(w) > 1 else np.empty(0, dtype=np.uint64)


def _needle_keys(arr):
    """secret rows (width a multiple of 4, at least 8) -> the uint64 of each of their 8-byte windows at 4-byte steps, zero windows dropped"""
    a = np.ascontiguousarray(arr, dtype=np.uint8)
    assert a.ndim == 2 and a.shape[1] >= 8 and a.shape[1] % 4 == 0, a.shape
    w = a.view("<u4").astype(np.uint64)
    k = (w[:, :-1] | (w[:, 1:] << np.uint64(32))).reshape(-1)
    return np.unique(k[k != 0])


def _find_needles(ws, needles):
    """-> [(buffer, secret, number of 8-byte windows of the buffer that equal a window of that secret)]: one vectorised membership test per pair"""
    hits = []
    for bname, buf in ws.items():
        if not buf.any():
            continue
        keys = _keys(buf)
        keys = keys[keys != 0]
        for nname, arr in needles.items():
            k = int(np.isin(keys, _needle_keys(arr)).sum())
            if k:
                hits.append((bname, nname, k))
    return hits


def _residue(ws, allow):
    """-> {buffer: count of non-zero bytes that no allowed public content explains}.  allow: {buffer: [(what, why public, bytes)]}: each content is looked
    for as ONE contiguous run (the staging layouts are contiguous per array) and blanked where found"""
    left = {}
    for bname, buf in ws.items():
        b = buf.copy()
        raw = b.tobytes()
        for what, why, content in allow.get(bname, []):
            if callable(content):                             # a value the test cannot compute: content(buffer) -> (first, end) of the bytes it explains, after checking them
                lo, hi = content(buf)
                b[lo:hi] = 0
                continue
            c = np.ascontiguousarray(content).view(np.uint8).reshape(-1).tobytes()
            at = raw.find(c) if c else -1
            if at >= 0:
                b[at:at + len(c)] = 0
        if b.any():
            left[bname] = (int(np.count_nonzero(b)), int(np.flatnonzero(b)[0]), int(np.flatnonzero(b)[-1]))
    return left


def _judge(eng, needles, allow, label):
    eng.synchronize()
    ws = eng.workspaces()
    hits = _find_needles(ws, needles)
    left = _residue(ws, allow)
    print("%s: workspaces %s; secrets found %s; unexplained non-zero bytes (count, first, last) %s"
          % (label, {k: len(v) for k, v in ws.items() if len(v)}, hits, left))
    assert not hits, (label, "secret bytes left in a workspace (buffer, secret, rows)", hits)
    assert not left, (label, "non-zero bytes outside the allow-list of public leftovers", left)


def _idx(n, few=None):
    """the items whose result is compared with the oracle: all of a small batch (the first `few` where the oracle is a Python loop); of a large one the ends,
    a seeded sample, and both sides of every multiple of 1024 near the middle (ffi_chunk_units rounds the chunk size up to one)"""
    if n <= 5000:
        return np.arange(n if few is None else min(n, few))
    mid = [c + d for c in range((n // 2) & ~1023, n // 2 + 2049, 1024) for d in (-2, -1, 0, 1) if 0 <= c + d < n]
    return np.unique(np.concatenate([np.arange(8), np.arange(n - 8, n), np.array(mid), np.random.default_rng(n).integers(0, n, size=24 if few else 64)]))


def _points(eng, seed, n, fmt=E.FMT_RAW160):
    """n public points: multiples of B by public scalars"""
    return eng.mul_base_batch_vartime_t(_dev(rand_scalars(seed, n)), out_fmt=fmt).cpu().numpy()


# ---- the cases: f(eng, n, round) -> (needles {name: rows}, allow {buffer: [(what, why public, content)]}) after checking the result ---------------------
def case_mul_base_batch(eng, n, rnd):
    s = rand_scalars(100 + rnd, n)
    got = eng.mul_base_batch(s)
    i = _idx(n)
    assert np.array_equal(got[i], orc.mul_base_compress_batch(s[i], threads=4))
    return {"scalars": s}, {"tmp_b": [("s_i B encodings", "the call's output: public keys / commitments to publish", got)]}


def case_mul_base_batch_t(eng, n, rnd):
    s = rand_scalars(110 + rnd, n)
    got = eng.mul_base_batch_t(_dev(s)).cpu().numpy()
    assert np.array_equal(got, orc.mul_base_compress_batch(s, threads=4))
    return {"scalars": s}, {}


def case_mul_base_clamped_batch(eng, n, rnd):
    raw = rand_bytes(120 + rnd, n)
    got = eng.mul_base_clamped_batch(raw)
    i = _idx(n, 64)
    want = np.stack([np.frombuffer(orc.ed_compress(orc.ed_mul_base(c.tobytes())), dtype=np.uint8) for c in _clamp(raw)[i]])
    assert np.array_equal(got[i], want)
    return {"raw": raw, "clamped": _clamp(raw)}, {"tmp_b": [("clamp(k_i) B encodings", "the call's output: public keys", got)]}


def case_mul_table_batch(eng, n, rnd):
    P = _points(eng, 5131, 1, E.FMT_EDWARDS_Y)[0]
    h = eng.basetable_create(P.tobytes())
    try:
        s = rand_scalars(130 + rnd, n)
        got = eng.mul_table_batch(h, s)
        Praw = orc.ed_decompress(P.tobytes())
        i = _idx(n, 64)
        want = np.stack([np.frombuffer(orc.ed_compress(orc.ed_mul(Praw, x.tobytes())), dtype=np.uint8) for x in s[i]])
        assert np.array_equal(got[i], want)
    finally:
        eng.basetable_destroy(h)
    return {"scalars": s}, {"tmp_b": [("s_i P encodings", "the call's output for a public table point: commitments to publish", got)]}


def _mul_ok(got, s, pts):
    i = _idx(len(s), 48)
    return np.array_equal(got[i], np.stack([np.frombuffer(orc.ed_compress(orc.ed_mul(pts[j].tobytes(), s[j].tobytes())), dtype=np.uint8) for j in i]))


def case_mul_batch(eng, n, rnd):
    s = rand_scalars(140 + rnd, n); pts = _points(eng, 5141, n)
    got = eng.mul_batch(s, pts)
    got = got[0] if isinstance(got, tuple) else got
    assert _mul_ok(np.asarray(got), s, pts)
    return ({"scalars": s, "products": np.asarray(got)},
            {"tmp_b": [("the points", "public input", pts)], "tmp_c": [("decode flags", "whether a public point decodes", np.ones(n, dtype=np.uint8))]})


def case_mul_batch_t(eng, n, rnd):
    s = rand_scalars(150 + rnd, n); pts = _points(eng, 5151, n)
    got = eng.mul_batch_t(_dev(s), _dev(pts))
    got = (got[0] if isinstance(got, tuple) else got).cpu().numpy()
    assert _mul_ok(got, s, pts)
    return {"scalars": s, "products": got}, {}


def case_mul_clamped_batch(eng, n, rnd):
    raw = rand_bytes(160 + rnd, n); pts = _points(eng, 5161, n)
    got = eng.mul_clamped_batch(raw, pts)
    got = np.asarray(got[0] if isinstance(got, tuple) else got)
    assert _mul_ok(got, _clamp(raw), pts)
    return ({"raw": raw, "clamped": _clamp(raw), "products": got},
            {"tmp_b": [("the points", "public input", pts)], "tmp_c": [("decode flags", "whether a public point decodes", np.ones(n, dtype=np.uint8))]})


def case_x25519_batch(eng, n, rnd):
    k = rand_bytes(170 + rnd, n); u = rand_bytes(5171, n)
    got = eng.x25519_batch(k, u)
    i = _idx(n)
    assert np.array_equal(got[i], orc.x25519_batch(k[i], u[i], threads=4))
    return {"k": k, "clamped": _clamp(k), "shared": got}, {"tmp_b": [("u coordinates", "the peer's public key", u)]}


def case_x25519_batch_t(eng, n, rnd):
    k = rand_bytes(180 + rnd, n); u = rand_bytes(5181, n)
    got = eng.x25519_batch_t(_dev(k), _dev(u)).cpu().numpy()
    assert np.array_equal(got, orc.x25519_batch(k, u, threads=4))
    return {"k": k, "clamped": _clamp(k), "shared": got}, {}


def case_x25519_contributory_batch(eng, n, rnd):
    k = rand_bytes(190 + rnd, n); u = rand_bytes(5191, n)
    got, flags = eng.x25519_contributory_batch(k, u)
    i = _idx(n)
    assert np.array_equal(got[i], orc.x25519_batch(k[i], u[i], threads=4)) and np.asarray(flags).all()
    return ({"k": k, "clamped": _clamp(k), "shared": got},
            {"tmp_b": [("u coordinates", "the peer's public key", u)],
             "tmp_c": [("contributory flags", "1 per item for full-order public keys: reveals nothing of k", np.ones(n, dtype=np.uint8))]})


def _x_base_want(k):
    nine = np.zeros((k.shape[0], 32), dtype=np.uint8); nine[:, 0] = 9
    return orc.x25519_batch(k, nine, threads=4)


def case_x25519_base_batch(eng, n, rnd):
    k = rand_bytes(200 + rnd, n)
    got = eng.x25519_base_batch(k)
    i = _idx(n)
    assert np.array_equal(got[i], _x_base_want(k[i]))
    return {"k": k, "clamped": _clamp(k)}, {"tmp_b": [("public keys", "the call's output: X25519 public keys", got)]}


def case_x25519_base_batch_t(eng, n, rnd):
    k = rand_bytes(210 + rnd, n)
    got = eng.x25519_base_batch_t(_dev(k)).cpu().numpy()
    assert np.array_equal(got, _x_base_want(k))
    return {"k": k, "clamped": _clamp(k)}, {}


def _mont_ok(got, s, u):
    # got[i] = u(s_i * P_i) on the sample; u = None: the basepoint
    i = _idx(len(s), 48)
    nine = bytes([9]) + bytes(31)
    return np.array_equal(got[i], np.stack([np.frombuffer(orc.mont_mul(nine if u is None else u[j].tobytes(), s[j].tobytes()), dtype=np.uint8) for j in i]))


def case_montgomery_mul_batch(eng, n, rnd):
    s = rand_scalars(220 + rnd, n); u = rand_bytes(5221, n)
    got = eng.montgomery_mul_batch(s, u)
    assert _mont_ok(got, s, u)
    return {"scalars": s, "products": got}, {"tmp_b": [("u coordinates", "public input", u)]}


def case_montgomery_mul_batch_t(eng, n, rnd):
    s = rand_scalars(230 + rnd, n); u = rand_bytes(5231, n)
    got = eng.montgomery_mul_batch_t(_dev(s), _dev(u)).cpu().numpy()
    assert _mont_ok(got, s, u)
    return {"scalars": s, "products": got}, {}


def _bits_be(k):
    """bits 254..0 of the scalars, most significant first, packed: the 32-byte bit strings for which mul_bits_be is the scalar multiplication"""
    return np.packbits(np.unpackbits(k[:, ::-1], axis=1)[:, 1:], axis=1)


def case_montgomery_mul_bits_be_batch(eng, n, rnd):
    s = rand_scalars(225 + rnd, n); u = rand_bytes(5226, n); bits = _bits_be(s)
    got = eng.montgomery_mul_bits_be_batch(bits, 255, u)
    assert _mont_ok(got, s, u)
    return {"bit strings": bits, "scalars": s, "products": got}, {"tmp_b": [("u coordinates", "public input", u)]}


def case_montgomery_mul_bits_be_batch_t(eng, n, rnd):
    s = rand_scalars(235 + rnd, n); u = rand_bytes(5236, n); bits = _bits_be(s)
    got = eng.montgomery_mul_bits_be_batch_t(_dev(bits), 255, _dev(u)).cpu().numpy()
    assert _mont_ok(got, s, u)
    return {"bit strings": bits, "scalars": s, "products": got}, {}


def case_montgomery_mul_base_batch(eng, n, rnd):
    s = rand_scalars(240 + rnd, n)
    got = eng.montgomery_mul_base_batch(s)
    assert _mont_ok(got, s, None)
    return {"scalars": s}, {"tmp_b": [("s_i B u-coordinates", "the call's output: public keys", got)]}


def case_montgomery_mul_base_batch_t(eng, n, rnd):
    s = rand_scalars(250 + rnd, n)
    got = eng.montgomery_mul_base_batch_t(_dev(s)).cpu().numpy()
    assert _mont_ok(got, s, None)
    return {"scalars": s}, {}


def case_keygen_batch_t(eng, n, rnd):
    seeds = rand_bytes(260 + rnd, n)
    got = eng.keygen_batch_t(_dev(seeds)).cpu().numpy()
    a, prefix = _expand(seeds)
    assert np.array_equal(got, orc.mul_base_compress_batch(a, threads=4))          # (a < 2^255: the oracle multiplies the integer as it is)
    return {"seeds": seeds, "a": a, "prefix": prefix}, {}


def _sign_inputs(seed, n):
    seeds = rand_bytes(seed, n)
    lens = np.random.default_rng(seed + 1).integers(0, 200, size=n)
    blob = rand_bytes(seed + 2, int(lens.sum()) + 1, 1).reshape(-1)[:int(lens.sum())]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    msgs = [blob[off[i]:off[i + 1]].tobytes() for i in range(n)]
    return seeds, blob, off, msgs


def _sign_public(pks, sigs, msgs, dom=b""):
    """what signing may leave behind: the A || R encodings (contiguous: A rows then R rows) and the H(dom || R || A || M) digests"""
    AR = np.concatenate([pks, sigs[:, :32]])
    hram = np.frombuffer(b"".join(hashlib.sha512(dom + sigs[i, :32].tobytes() + pks[i].tobytes() + msgs[i]).digest() for i in range(len(msgs))), dtype=np.uint8)
    return [("A || R encodings", "public keys and the public half of the signatures", AR), ("H(R || A || M) digests", "a hash of public values", hram)]


def _sign_flag(n):
    """flag word 0 of a signing call: k_hram counts the non-canonical s halves it sees, and while it hashes R || A || M the s halves of the caller's
    output buffer are not written yet -- a count of whatever that buffer held before, at most n, and no function of any secret"""
    def explain(buf):
        assert int(np.frombuffer(buf[:4].tobytes(), dtype=np.uint32)[0]) <= n
        return 0, 4
    return ("count of non-canonical s halves seen by k_hram", "counts the not-yet-written halves of the caller's output buffer: no secret enters", explain)


def _sign_check(seeds, msgs, pks, sigs):
    for i in range(0, len(msgs), max(1, len(msgs) // 40)):
        assert pks[i].tobytes() == orc.ed25519_pubkey(seeds[i].tobytes()) and sigs[i].tobytes() == orc.ed25519_sign(seeds[i].tobytes(), msgs[i]), i


def _sign_needles(seeds, msgs, dom=b""):
    a, prefix = _expand(seeds)
    return {"seeds": seeds, "a": a, "prefix": prefix, "nonce r": _nonces(prefix, msgs, dom)}


def case_sign_batch_t(eng, n, rnd):
    seeds, blob, off, msgs = _sign_inputs(270 + 10 * rnd, n)
    pks, sigs = eng.sign_batch_t(_dev(seeds), _dev(blob) if len(blob) else torch.empty(0, dtype=torch.uint8, device="cuda"), _dev(off))
    pks, sigs = pks.cpu().numpy(), sigs.cpu().numpy()
    _sign_check(seeds, msgs, pks, sigs)
    return _sign_needles(seeds, msgs), {"tmp_f": _sign_public(pks, sigs, msgs), "d_flag": [_sign_flag(n)]}


def case_sign_batch(eng, n, rnd):
    seeds, blob, off, msgs = _sign_inputs(300 + 10 * rnd, n)
    pks, sigs = eng.sign_batch([s.tobytes() for s in seeds], msgs)
    _sign_check(seeds, msgs, pks, sigs)
    return (_sign_needles(seeds, msgs),
            {"tmp_f": _sign_public(pks, sigs, msgs), "d_flag": [_sign_flag(n)], "tmp_a": [("the messages", "public input", blob)], "tmp_b": [("message offsets", "public input", off.astype(np.uint64))],
             "tmp_c": [("public keys", "the call's output", pks), ("signatures", "the call's output", sigs)]})


def _ph_inputs(seed, n):
    seeds = rand_bytes(seed, n); ph = rand_bytes(seed + 1, n, 64)
    ctxt = b"wipe test context"
    dom = b"SigEd25519 no Ed25519 collisions" + bytes([1, len(ctxt)]) + ctxt
    return seeds, ph, ctxt, dom


def _ph_check(seeds, ph, ctxt, pks, sigs):
    for i in range(0, len(seeds), max(1, len(seeds) // 40)):
        assert (0, sigs[i].tobytes()) == tuple(orc.ed25519_sign_prehashed(seeds[i].tobytes(), ph[i].tobytes(), ctxt)), i


def case_sign_batch_prehashed_t(eng, n, rnd):
    seeds, ph, ctxt, dom = _ph_inputs(330 + 10 * rnd, n)
    pks, sigs = eng.sign_batch_prehashed_t(_dev(seeds), _dev(ph), ctxt)
    pks, sigs = pks.cpu().numpy(), sigs.cpu().numpy()
    _ph_check(seeds, ph, ctxt, pks, sigs)
    msgs = [p.tobytes() for p in ph]
    return (_sign_needles(seeds, msgs, dom),
            {"tmp_f": _sign_public(pks, sigs, msgs, dom), "d_flag": [_sign_flag(n)], "dom": [("dom2", "the public domain separator and context", np.frombuffer(dom, dtype=np.uint8))]})


def case_sign_batch_prehashed(eng, n, rnd):
    seeds, ph, ctxt, dom = _ph_inputs(360 + 10 * rnd, n)
    pks, sigs = eng.sign_batch_prehashed([x.tobytes() for x in seeds], [x.tobytes() for x in ph], ctxt)
    pks, sigs = np.asarray(pks), np.asarray(sigs)
    _ph_check(seeds, ph, ctxt, pks, sigs)
    msgs = [p.tobytes() for p in ph]
    return (_sign_needles(seeds, msgs, dom),
            {"tmp_f": _sign_public(pks, sigs, msgs, dom), "d_flag": [_sign_flag(n)], "dom": [("dom2", "the public domain separator and context", np.frombuffer(dom, dtype=np.uint8))],
             "tmp_a": [("the prehashes", "public input: digests of the messages", ph)],
             "tmp_c": [("public keys", "the call's output", pks), ("signatures", "the call's output", sigs)]})


def case_msm_consttime(eng, n, rnd):
    s = rand_scalars(390 + rnd, n); pts = _points(eng, 5391, n)
    st, got = eng.msm_consttime(s, pts)
    want = orc.ed_compress(orc.ed_msm([x.tobytes() for x in s], [p.tobytes() for p in pts]))
    assert st == 0 and got == want
    return ({"scalars": s},
            {"tmp_b": [("the points", "public input", pts)], "tmp_c": [("decode flags", "whether a public point decodes", np.ones(n, dtype=np.uint8))]})


def case_scalar_invert_batch(eng, n, rnd):
    s = rand_scalars(400 + rnd, n); s[:, 0] |= 1
    inv, prod = eng.scalar_invert_batch(s)
    for i in range(0, n, max(1, n // 64)):
        assert int.from_bytes(inv[i].tobytes(), "little") * int.from_bytes(s[i].tobytes(), "little") % L == 1, i
    return {"scalars": s, "inverses": inv}, {}


def case_lizard_encode_batch(eng, n, rnd):
    data = rand_bytes(410 + rnd, n, 16)
    pts = eng.ristretto_lizard_encode_batch(data)
    back = _on_other_engine(lambda o: o.ristretto_lizard_decode_batch(pts))[0]
    assert np.array_equal(np.asarray(back), data)             # (the decode path has its own oracle tests: tests/test_gpu_lizard.py; here the round trip shows the work was done)
    return {"payloads": data, "points": np.asarray(pts)}, {}


def case_lizard_encode_batch_t(eng, n, rnd):
    data = rand_bytes(420 + rnd, n, 16)
    pts = eng.ristretto_lizard_encode_batch_t(_dev(data))
    back = _on_other_engine(lambda o: o.ristretto_lizard_decode_batch_t(pts))[0]
    assert np.array_equal(back.cpu().numpy(), data)
    return {"payloads": data, "points": pts.cpu().numpy()}, {}


def _on_other_engine(f):
    """f(engine) on an engine of its own, so that the engine under test runs the call under test and nothing else"""
    other = pkg.Engine(0)
    try:
        return f(other)
    finally:
        other.close()


def case_lizard_decode_batch(eng, n, rnd):
    data = rand_bytes(450 + rnd, n, 16); pts = _on_other_engine(lambda o: np.asarray(o.ristretto_lizard_encode_batch(data)))
    out, st = eng.ristretto_lizard_decode_batch(pts)
    assert np.array_equal(np.asarray(out), data) and np.asarray(st).all()      # (the encoder against the oracle: tests/test_gpu_lizard.py)
    return {"payloads": data, "points": pts}, {"tmp_c": [("decode status", "1 per item: every point carries exactly one payload", np.ones(n, dtype=np.uint8))]}


def case_lizard_decode_batch_t(eng, n, rnd):
    data = rand_bytes(460 + rnd, n, 16); pts = _on_other_engine(lambda o: np.asarray(o.ristretto_lizard_encode_batch(data)))
    out, st = eng.ristretto_lizard_decode_batch_t(_dev(pts))
    assert np.array_equal(out.cpu().numpy(), data) and bool(st.all())
    return {"payloads": data, "points": pts}, {}


def case_from_uniform_bytes_batch_t(eng, n, rnd):
    u = rand_bytes(470 + rnd, n, 64)
    got = eng.ristretto_from_uniform_bytes_batch_t(_dev(u)).cpu().numpy()
    assert np.array_equal(got, _on_other_engine(lambda o: o.ristretto_from_uniform_bytes_batch(u)))      # (oracle parity: tests/test_gpu_h2c.py)
    return {"uniform bytes": u, "points": got}, {}


def case_map_to_curve_batch_t(eng, n, rnd):
    u = rand_bytes(480 + rnd, n)
    got = eng.ristretto_map_to_curve_batch_t(_dev(u)).cpu().numpy()
    assert np.array_equal(got, _on_other_engine(lambda o: o.ristretto_map_to_curve_batch(u)))
    return {"field bytes": u, "points": got}, {}


def case_from_uniform_bytes_batch(eng, n, rnd):
    u = rand_bytes(430 + rnd, n, 64)
    got = eng.ristretto_from_uniform_bytes_batch(u)
    assert np.array_equal(got, _on_other_engine(lambda o: o.ristretto_from_uniform_bytes_batch_t(_dev(u)).cpu().numpy()))     # (oracle parity: tests/test_gpu_h2c.py)
    return {"uniform bytes": u, "points": np.asarray(got)}, {}


def case_map_to_curve_batch(eng, n, rnd):
    u = rand_bytes(440 + rnd, n)
    got = eng.ristretto_map_to_curve_batch(u)
    assert np.array_equal(got, _on_other_engine(lambda o: o.ristretto_map_to_curve_batch_t(_dev(u)).cpu().numpy()))
    return {"field bytes": u, "points": np.asarray(got)}, {}


CASES = [case_mul_base_batch, case_mul_base_batch_t, case_mul_base_clamped_batch, case_mul_table_batch, case_mul_batch, case_mul_batch_t, case_mul_clamped_batch,
         case_x25519_batch, case_x25519_batch_t, case_x25519_contributory_batch, case_x25519_base_batch, case_x25519_base_batch_t,
         case_montgomery_mul_batch, case_montgomery_mul_batch_t, case_montgomery_mul_bits_be_batch, case_montgomery_mul_bits_be_batch_t,
         case_montgomery_mul_base_batch, case_montgomery_mul_base_batch_t,
         case_keygen_batch_t, case_sign_batch_t, case_sign_batch, case_sign_batch_prehashed_t, case_sign_batch_prehashed,
         case_msm_consttime, case_scalar_invert_batch, case_lizard_encode_batch, case_lizard_encode_batch_t, case_lizard_decode_batch, case_lizard_decode_batch_t,
         case_from_uniform_bytes_batch, case_from_uniform_bytes_batch_t, case_map_to_curve_batch, case_map_to_curve_batch_t]
# host forms that run through ffi_twin, by the minimum chunk it is given (csrc: the 1u << k of each call): one chunk up to 2 * minimum, two above
CHUNKED = {1 << 16: [case_mul_batch, case_mul_clamped_batch, case_lizard_encode_batch, case_lizard_decode_batch, case_from_uniform_bytes_batch, case_map_to_curve_batch],
           1 << 17: [case_x25519_batch, case_x25519_contributory_batch, case_montgomery_mul_batch, case_montgomery_mul_bits_be_batch],
           1 << 18: [case_mul_base_batch, case_mul_base_clamped_batch, case_mul_table_batch, case_x25519_base_batch, case_montgomery_mul_base_batch]}

# every case at the first size; the ones that end in the Edwards compressor also either side of its 4096-point switch; the chunked host forms either side of
# their two-chunk threshold; x25519_batch also where its chunks are tapered (n >= 2^19)
PARAMS = ([(c, SIZES[0]) for c in CASES]
          + [(c, n) for c in (case_mul_base_batch, case_mul_batch_t, case_sign_batch_t, case_scalar_invert_batch, case_msm_consttime) for n in SIZES[1:]]
          + [(c, n) for m, cs in CHUNKED.items() for c in cs for n in (2 * m - 1, 2 * m + 1)]
          + [(case_x25519_batch, (1 << 19) + 1)])


@pytest.mark.parametrize("case,n", PARAMS, ids=["%s-%d" % (c.__name__[5:], n) for c, n in PARAMS])
def test_no_secret_stays_behind(case, n):
    eng = pkg.Engine(0)
    try:
        case(eng, n, 0)
        eng.workspace_zero()
        needles, allow = case(eng, n, 1)
        _judge(eng, needles, allow, "%s n=%d" % (case.__name__[5:], n))
    finally:
        eng.close()


def test_late_argument_error_leaves_nothing():
    """sign_batch_t with non-monotone offsets: the error flag is read back after the seeds were expanded and the nonces hashed -- EngineError, the
    workspaces hold no secret, and the next good call on the same engine is still correct"""
    n = 2048
    eng = pkg.Engine(0)
    try:
        case_sign_batch_t(eng, n, 0)
        eng.workspace_zero()
        seeds, blob, off, msgs = _sign_inputs(777, n)
        bad = off.copy(); bad[n // 2] = bad[n // 2 + 1] + 5      # offset i beyond offset i + 1
        with pytest.raises(E.EngineError):
            eng.sign_batch_t(_dev(seeds), _dev(blob), _dev(bad))
        eng.synchronize()
        ws = eng.workspaces()
        # what the kernels saw: an item whose offsets are out of order is hashed as the empty message
        msgs_seen = [blob[bad[i]:bad[i + 1]].tobytes() if bad[i] <= bad[i + 1] else b"" for i in range(n)]
        needles = _sign_needles(seeds, msgs_seen)
        hits = _find_needles(ws, needles)
        assert not hits, hits
        # zero elsewhere, as on the good path: tmp_f may hold the A || R encodings and the digests, both computed here from the seeds (the caller's outputs
        # are not to be trusted after an error); d_flag its two words; every other byte of every workspace is zero -- a || r || prefix among them
        pks = orc.mul_base_compress_batch(needles["a"], threads=4); R = orc.mul_base_compress_batch(needles["nonce r"], threads=4)
        sigs = np.concatenate([R, np.zeros((n, 32), dtype=np.uint8)], axis=1)

        def flags(buf):
            w = np.frombuffer(buf[:8].tobytes(), dtype=np.uint32)
            assert int(w[0]) <= n and int(w[1]) == 1, w
            return 0, 8
        left = _residue(ws, {"tmp_f": _sign_public(pks, sigs, msgs_seen),
                             "d_flag": [("flag words", "[0] counts s halves of the caller's unwritten output buffer, [1] = 1: the offsets were bad", flags)]})
        assert not left, left
        case_sign_batch_t(eng, n, 2)
    finally:
        eng.close()


def test_vartime_context_results_equal():
    """a context created with FLAG_VARTIME_TABLES declares its scalars public: same results, no wipe claim"""
    n = 1024
    ev = pkg.Engine(0, flags=E.FLAG_VARTIME_TABLES); ec = pkg.Engine(0)
    try:
        s = rand_scalars(900, n); seeds, blob, off, msgs = _sign_inputs(901, n)
        assert np.array_equal(ev.mul_base_batch(s), ec.mul_base_batch(s))
        a = ev.sign_batch_t(_dev(seeds), _dev(blob), _dev(off)); b = ec.sign_batch_t(_dev(seeds), _dev(blob), _dev(off))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    finally:
        ev.close(); ec.close()
