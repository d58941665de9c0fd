"""Edge ENCODINGS through the MSM over compressed input (in_fmt 0 / 1): every distinct key and R of the Ed25519 edge-case corpus that decodes, the eight torsion
points with their non-canonical twins (y + p, x = 0 with the sign bit set), the identity and ordinary encodings, tiled and shuffled to every size at which the
call changes path.  test_gpu_msm.py feeds these paths random encodings -- canonical and of large order with probability 1 - 2^-250.  Every sum is judged by
the oracle's MSM over the oracle's own decompression of the same encodings (these points are no multiples of B: no sum-of-squares identity applies)."""
import os
import subprocess
import textwrap

import numpy as np
import pytest

import corpus
import util

pytestmark = pytest.mark.gpu
ED, RIS, RAW = 0, 1, 2
# 1000 / 4095: the small path; 4096 / 5000 / 6143: the mid path with the 12-bit layout; 6144 / 16391 / 65536 / 262144: the mid path, padded and unpadded digit rows, both
# ends; 262145: the bucket pipeline
SIZES = (1000, 4095, 4096, 5000, 6143, 6144, 16391, 65536, 262144, 262145)
HOST_SIZES = (4096, 65536)
RAW_SIZES = (6144, 262145)
BAD_SIZES = (4096, 6144, 262145)


@pytest.fixture(scope="module")
def eng():
    import curve25519_dalek_amd as pkg
    return pkg.Engine(0)


_TERMS = {}


def _terms(orc, n):
    """-> (scalars, encodings, the oracle's points, the oracle's sum as a 160-byte point) of size n, made once"""
    if n not in _TERMS:
        s, enc, dec = corpus.msm_terms(orc, n, 9000 + n)
        _TERMS[n] = (s, enc, dec, orc.ed_msm_mt_np(s, dec, threads=corpus.THREADS) if n >= 4096 else orc.ed_msm_np(s, dec))
    return _TERMS[n]


def _dev(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


@pytest.mark.parametrize("n", SIZES)
def test_edge_encodings_device_pointers(eng, orc, n):
    s, enc, dec, want = _terms(orc, n)
    ds, de = _dev(s, enc)
    st, got = eng.msm_vartime_t(ds, de, in_fmt=ED, out_fmt=ED)
    assert st == 0 and got == orc.ed_compress(want)
    st, got = eng.msm_vartime_t(ds, de, in_fmt=ED, out_fmt=RAW)
    assert st == 0 and orc.ed_eq(got, want)
    if n in RAW_SIZES:                                       # the same points as RAW160 (Z = 1): the direct normaliser sees x = 0 and y = 0 points
        st, got = eng.msm_vartime_t(ds, _dev(dec)[0], in_fmt=RAW, out_fmt=ED)
        assert st == 0 and got == orc.ed_compress(want)
    if n in BAD_SIZES:                                       # one encoding that is on no curve point: Option::None
        for at in (0, n // 2 + 1, n - 1):
            e2 = enc.copy()
            e2[at] = np.frombuffer(corpus.bad_point_encoding(orc), np.uint8)
            st, _ = eng.msm_vartime_t(ds, _dev(e2)[0], in_fmt=ED, out_fmt=ED)
            assert st == 1, at


@pytest.mark.parametrize("n", HOST_SIZES)
def test_edge_encodings_host_pointers(eng, orc, n):
    s, enc, dec, want = _terms(orc, n)
    st, got = eng.msm_vartime(s, enc, in_fmt=ED, out_fmt=ED)
    assert st == 0 and got == orc.ed_compress(want)


@pytest.mark.parametrize("n", BAD_SIZES)
def test_ristretto_encodings_and_one_the_decoder_refuses(eng, orc, n):
    """valid Ristretto encodings (of the doubles of the pool's points: torsion points double into the identity's coset) and, in a second call, one non-canonical s"""
    _, pool_dec, _ = corpus.point_pool(orc)
    base = [orc.ris_compress(orc.ed_double(pool_dec[i].tobytes())) for i in range(0, pool_dec.shape[0], 3)]
    base = sorted(set(base))
    dec1 = [orc.ris_decompress(e) for e in base]
    assert all(d is not None for d in dec1) and corpus.i2b(0) in base and len(base) >= 100
    rng = np.random.default_rng(4000 + n)
    idx = np.resize(np.arange(len(base)), n)
    rng.shuffle(idx)
    enc = np.frombuffer(b"".join(base), np.uint8).reshape(-1, 32)[idx]
    dec = np.frombuffer(b"".join(dec1), np.uint8).reshape(-1, 160)[idx]
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x7F
    want = orc.ris_compress(orc.ed_msm_mt_np(s, dec, threads=corpus.THREADS))
    ds, de = _dev(s, enc)
    st, got = eng.msm_vartime_t(ds, de, in_fmt=RIS, out_fmt=RIS)
    assert st == 0 and got == want
    bad = corpus.i2b(util.P)                                 # s = p: a non-canonical 0 (tests/test_gpu_group.py test_bad_ristretto_encodings)
    assert orc.ris_decompress(bad) is None
    for at in (0, n - 1):
        e2 = enc.copy()
        e2[at] = np.frombuffer(bad, np.uint8)
        st, _ = eng.msm_vartime_t(ds, _dev(e2)[0], in_fmt=RIS, out_fmt=RIS)
        assert st == 1, at


@pytest.mark.parametrize("knob", ["C25519_MSM_MID_MAX", "C25519_MSM_MID_MAX_RECORDS"])
def test_edge_encodings_with_the_mid_path_off(orc, knob):
    """4096 .. 6143 encoded terms take the 12-bit layout; with the mid path off (either knob of the tuning build) the bucket pipeline serves them with it --
    a size it otherwise never runs at, and test_gpu_msm.py only sends it raw points there"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = textwrap.dedent("""
        import sys, numpy as np
        sys.path.insert(0, %r); sys.path.insert(0, %r)
        import corpus, curve25519_dalek_amd as pkg
        from oracle import orc
        eng = pkg.Engine(0)
        for n in (4096, 5000, 6143):
            s, enc, dec = corpus.msm_terms(orc, n, 9000 + n)
            want = orc.ed_compress(orc.ed_msm_np(s, dec))
            st, got = eng.msm_vartime(s, enc, in_fmt=0, out_fmt=0)
            assert st == 0 and got == want, n
            e2 = enc.copy(); e2[n - 2] = np.frombuffer(corpus.bad_point_encoding(orc), np.uint8)
            assert eng.msm_vartime(s, e2, in_fmt=0, out_fmt=0)[0] == 1, n
        print("ok")
    """) % (here, os.path.dirname(here))
    r = subprocess.run(util.child_argv(code), env=util.tune_env({knob: "0"}), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (knob, r.stdout[-500:], r.stderr[-2000:])


def test_edge_encodings_through_the_segmented_msm(eng, orc):
    """one call: sums of 1, 2, 17, 64 terms (one lane each) and of 65, 300, 2048 terms (one wave each) over the pool; then one undecodable encoding in a lane
    segment and in a wave segment -- that segment alone reports it"""
    lengths = [1, 2, 17, 64, 65, 300, 2048, 64, 65]
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    n = int(off[-1])
    s, enc, dec = corpus.msm_terms(orc, n, 77)
    want = [orc.ed_compress(orc.ed_msm_np(s[int(a):int(b)], dec[int(a):int(b)])) for a, b in zip(off[:-1], off[1:])]
    plan = eng.msm_vartime_segments_plan(off)
    assert plan[0] == 5 and plan[1] == 4 and plan[2] == 0
    st, out, ok = eng.msm_vartime_segments(s, enc, off, ED, ED)
    assert st == 0 and ok.all()
    assert [k for k in range(len(lengths)) if out[k].tobytes() != want[k]] == []
    for seg in (2, 5):
        e2 = enc.copy()
        e2[int(off[seg]) + lengths[seg] // 2] = np.frombuffer(corpus.bad_point_encoding(orc), np.uint8)
        st, out, ok = eng.msm_vartime_segments(s, e2, off, ED, ED)
        assert st == 1
        assert [int(x) for x in ok] == [int(k != seg) for k in range(len(lengths))]
        assert [k for k in range(len(lengths)) if k != seg and out[k].tobytes() != want[k]] == []
