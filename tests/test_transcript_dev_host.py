"""The per-lane Merlin transcript of the segmented verify_batch (curve25519-dalek_amd/csrc/transcript_dev.h), without a GPU:
  - the header built for the host (tests/host/transcript_dev_host.cpp) against the library's host transcript for every segment length 0 .. 200 --
    the hram phase advances 76 bytes per signature (all 83 alignments against the 166-byte block), the sig.s phase 45 bytes (all 166), so every
    header, label, length and data piece is split by a block boundary somewhere in that range -- and against the independent STROBE of tests/pyref.py;
  - the same program stand-alone under AddressSanitizer + UBSan on exactly-sized heap buffers;
  - ed25519_batch_transcript_zs_segments_plan: which transcripts ed25519_verify_batch_segments runs on the device and which on the host;
  - the compiled kernel: k_mid_vseg_transcript exists, has no private segment and no scratch traffic."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pyref
from util import asm_kernels, demangle_kernel, device_asm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "transcript_dev_host.cpp")
DEPS = [SRC] + [os.path.join(ROOT, "curve25519-dalek_amd", "csrc", f) for f in ("transcript_dev.h", "transcript_host.h", "constants_gen.h")]


@pytest.fixture(scope="module")
def pkg():
    import curve25519_dalek_amd as p
    p.load_library()
    return p


@pytest.fixture(scope="module")
def host():
    so = os.path.join(ROOT, "tests", "host", "libtranscriptdevhost.so")
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in DEPS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, SRC])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def rows():
    """random hram and signature rows (no valid signatures are needed: the transcript absorbs bytes), shared and never written"""
    rng = np.random.default_rng(2024)
    h = rng.integers(0, 256, size=(200, 64), dtype=np.uint8)
    s = rng.integers(0, 256, size=(200, 64), dtype=np.uint8)
    h.setflags(write=False); s.setflags(write=False)
    return h, s


def _dev_zs(host, h, s):
    n = h.shape[0]
    z = np.full((n + 1, 16), 0xA5, dtype=np.uint8)          # (a guard row behind the last)
    hc, sc = np.ascontiguousarray(h), np.ascontiguousarray(s)
    host.h_transcript_dev_zs(C.c_void_p(hc.ctypes.data), C.c_void_p(sc.ctypes.data), C.c_uint64(n), C.c_void_p(z.ctypes.data))
    assert (z[n] == 0xA5).all()
    return z[:n]


def test_every_length_equals_the_host_transcript(pkg, host, rows):
    h, s = rows
    for n in range(0, 201):
        # (a different window of the rows per length: the data pieces differ as well as the alignments)
        a = (7 * n) % (200 - n + 1)
        got = _dev_zs(host, h[a:a + n], s[a:a + n])
        want = pkg.engine.batch_transcript_zs(h[a:a + n], s[a:a + n])
        assert np.array_equal(got, want), n


def test_short_lengths_equal_the_independent_strobe(host, rows):
    h, s = rows
    for n in (0, 1, 2, 3, 7, 40):
        got = _dev_zs(host, h[:n], s[:n])
        want = pyref.batch_transcript_zs([h[i].tobytes() for i in range(n)], [s[i, 32:].tobytes() for i in range(n)])
        assert [got[i].tobytes() for i in range(n)] == list(want), n


def test_stand_alone_under_asan_ubsan(tmp_path):
    """nothing is loaded into python: the harness has a main of its own that compares lengths 0 .. 400 with csrc/transcript_host.h"""
    exe = str(tmp_path / "transcript_dev_san")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17", "-Wno-unknown-pragmas",
                           "-DTRANSCRIPT_DEV_MAIN", SRC, "-o", exe])
    env = dict(os.environ); env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=1"; env["UBSAN_OPTIONS"] = "halt_on_error=1"
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "sanitized ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def _off(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.uint64))]).astype(np.uint64)


def test_plan_counts(pkg):
    E = pkg.Engine
    T, seg_max = pkg.engine.TRANSCRIPT_SEGMENT_DEVICE_MAX, pkg.engine.VERIFY_SEGMENT_MAX
    assert 0 <= T <= seg_max == 1023
    lens = [0, 1, T, T + 1, 1023, 1024, 5000]
    dev = sum(1 for l in lens if l <= T)
    host_side = sum(1 for l in lens if T < l <= seg_max)
    assert E.batch_transcript_zs_segments_plan(_off(lens)) == (dev, host_side)
    assert dev + host_side == sum(1 for l in lens if l <= seg_max)
    assert E.batch_transcript_zs_segments_plan(_off([])) == (0, 0)
    assert E.batch_transcript_zs_segments_plan(_off([2000])) == (0, 0)
    assert E.batch_transcript_zs_segments_plan(_off([0, 0, 0])) == (3, 0)
    # the two plans agree on which segments are on the segmented route at all
    assert sum(E.batch_transcript_zs_segments_plan(_off(lens))) == E.verify_batch_segments_plan(_off(lens))[0]


def test_plan_rejects_bad_offsets(pkg):
    E = pkg.Engine
    for bad in ([0, 5, 3, 7], [1, 2, 3], [0, 1 << 40]):
        with pytest.raises(pkg.EngineError):
            E.batch_transcript_zs_segments_plan(np.array(bad, dtype=np.uint64))
        with pytest.raises(pkg.EngineError):
            E.verify_batch_segments_plan(np.array(bad, dtype=np.uint64))
    lib = pkg.load_library()
    two = np.zeros(2, dtype=np.uint64)
    plan = np.zeros(2, dtype=np.uint64)
    for m in (0xffffffff, 1 << 33):                         # refused before seg_off[m] is read: two readable offsets only
        assert lib.ed25519_batch_transcript_zs_segments_plan(two.ctypes.data, C.c_uint64(m), plan.ctypes.data) == -1      # -(hipErrorInvalidValue)
    assert lib.ed25519_batch_transcript_zs_segments_plan(None, C.c_uint64(3), plan.ctypes.data) == -1


def test_header_constant_matches_python(pkg):
    import re
    hdr = open(os.path.join(ROOT, "include", "c25519_hip.h")).read()
    m = re.search(r"#define\s+ED25519_TRANSCRIPT_SEGMENT_DEVICE_MAX\s+(\d+)", hdr)
    assert m and int(m.group(1)) == pkg.engine.TRANSCRIPT_SEGMENT_DEVICE_MAX


def test_compiled_kernel_keeps_the_sponge_in_registers(tmp_path_factory):
    kernels = asm_kernels(device_asm(tmp_path_factory, "verify_seg"))
    mine = {sym: v for sym, v in kernels.items() if (demangle_kernel(sym) or "").startswith("k_mid_vseg_transcript")}
    assert len(mine) == 1, sorted(kernels)
    (body, priv), = mine.values()
    assert priv == 0
    assert not [l for l in body if "scratch_" in l]
