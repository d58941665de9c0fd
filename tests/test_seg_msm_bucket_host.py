"""The bucket route of the segmented vartime MSM (csrc/mid_segb.hip) as far as a machine without a GPU can see it: the per-segment routing
function c25519_msm_vartime_segments_routes (host arithmetic; the call itself routes with the same code) beside the plan function, its
binding, the two constants of the header, and the route's digit recoding (csrc/segb_digits.h) stand-alone against Python integers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES, PLAN = "c25519_msm_vartime_segments_routes", "c25519_msm_vartime_segments_plan"
INVALID = -1                                                 # -(hipErrorInvalidValue)
LANE, WAVE, BUCKET, SINGLE = 0, 1, 2, 3


def _header_constant(name):
    hdr = open(os.path.join(ROOT, "include", "c25519_hip.h")).read()
    m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, hdr, flags=re.M)
    assert m, "%s is not defined in include/c25519_hip.h" % name
    return int(m.group(1))


def _consts():
    import curve25519_dalek_amd as pkg
    e = pkg.engine
    return e.MSM_SEGMENT_DIRECT_MAX, e.MSM_SEGMENT_WAVE_MAX, e.MSM_SEGMENT_BUCKET_MAX, e.MSM_SEGMENT_BUCKET_PASS_TERMS


def _off(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.uint64))]).astype(np.uint64)


def _call(name, off, m, out):
    import curve25519_dalek_amd as pkg
    off = np.ascontiguousarray(np.asarray(off, dtype=np.uint64))
    return getattr(pkg.load_library(), name)(off.ctypes.data if off.size else None, len(off) - 1 if m is None else m, out.ctypes.data)


def _routes_raw(off, m=None):
    """-> (status, routes) of the C function on the offsets as given (no checks on this side)"""
    route = np.full(max(1, len(off)), 0xEE, np.uint8)
    st = _call(ROUTES, off, m, route)
    return st, [int(x) for x in route[:(len(off) - 1 if m is None else m)]]


def _plan_raw(off, m=None):
    plan = np.full(5, 0xEE, np.uint64)
    st = _call(PLAN, off, m, plan)
    return st, tuple(int(x) for x in plan)


# ---- export and binding ---------------------------------------------------------------------------------------------------------
def test_library_exports_and_engine_binds_the_routes_function():
    import curve25519_dalek_amd as pkg
    assert hasattr(pkg.load_library(), ROUTES), "libc25519hip.so does not export %s" % ROUTES
    assert ROUTES in pkg.engine._SIGS and ROUTES in pkg.engine.ABI_SYMBOLS
    res, args = pkg.engine._SIGS[ROUTES]
    assert res is C.c_int32 and len(args) == 3 and args[1] is C.c_uint64      # seg_off, m, route
    assert callable(pkg.Engine.msm_vartime_segments_routes)
    e = pkg.engine
    assert (e.MSM_SEGMENT_ROUTE_LANE, e.MSM_SEGMENT_ROUTE_WAVE, e.MSM_SEGMENT_ROUTE_BUCKET, e.MSM_SEGMENT_ROUTE_SINGLE) == (LANE, WAVE, BUCKET, SINGLE)
    for k, name in enumerate(("LANE", "WAVE", "BUCKET", "SINGLE")):
        assert _header_constant("C25519_MSM_SEGMENT_ROUTE_" + name) == k


def test_bucket_constants_are_the_engines_and_in_order():
    D, W, B, BT = _consts()
    assert _header_constant("C25519_MSM_SEGMENT_BUCKET_MAX") == B and _header_constant("C25519_MSM_SEGMENT_BUCKET_PASS_TERMS") == BT
    assert BT >= B > W and B <= 65536                        # one segment always fits into a pass; a term index within its segment is 16 bits
    # the workspace of a full bucket pass (257 bytes per term, 5152 per segment of more than WAVE_MAX terms) stays within that of a Straus pass
    import curve25519_dalek_amd as pkg
    assert BT * 257 + (BT // (W + 1)) * 5152 <= pkg.engine.MSM_SEGMENT_PASS_TERMS * 1345 + 4096


# ---- the routes on hand-made offsets --------------------------------------------------------------------------------------------
def test_routes_at_every_boundary():
    D, W, B, BT = _consts()
    assert (D, W) == (64, 2048)
    lengths = [0, 1, 64, 65, 2048, 2049, B, B + 1]
    st, routes = _routes_raw(_off(lengths))
    assert st == 0 and routes == [LANE, LANE, LANE, WAVE, WAVE, BUCKET, BUCKET, SINGLE]
    import curve25519_dalek_amd as pkg
    got = pkg.Engine.msm_vartime_segments_routes(_off(lengths))
    assert got.dtype == np.uint8 and got.tolist() == routes


def test_routes_degenerate_and_rejected_offsets():
    assert _routes_raw([0], 0) == (0, [])                   # m = 0
    assert _routes_raw([], 0) == (0, [])                    # ... where seg_off may be null, as in the call
    assert _routes_raw([0, 0, 0]) == (0, [LANE, LANE])
    for bad in ([1, 2, 4], [0, 3, 2, 4], [0, 2, 1], [0, 5, 1 << 40]):
        st, _ = _routes_raw(bad)
        assert st == INVALID and _plan_raw(bad)[0] == st, (bad, st)
    st, _ = _routes_raw([], 3)                               # null offsets with m > 0
    assert st == INVALID and _plan_raw([], 3)[0] == st
    import curve25519_dalek_amd as pkg
    with pytest.raises(pkg.engine.EngineError):
        pkg.Engine.msm_vartime_segments_routes([0, 3, 2])


def test_route_counts_are_the_plans_on_random_offsets():
    D, W, B, BT = _consts()
    rng = np.random.default_rng(32)
    edges = [0, 1, D - 1, D, D + 1, W - 1, W, W + 1, 2 * W, B - 1, B, B + 1, 2 * B]
    for case in range(200):
        m = int(rng.integers(1, 300))
        kind = case % 4
        if kind == 0:
            lengths = rng.integers(0, 2 * D, size=m)
        elif kind == 1:
            lengths = rng.choice(edges, size=m)
        elif kind == 2:
            lengths = np.where(rng.random(m) < 0.1, B + 1 + rng.integers(0, 100, size=m), rng.integers(W // 2, 2 * W, size=m))
        else:
            lengths = np.where(rng.random(m) < 0.5, rng.integers(0, W + 1, size=m), rng.integers(W + 1, B + 2, size=m))
        lengths = [int(x) for x in lengths]
        off = _off(lengths)
        st, routes = _routes_raw(off)
        st2, plan = _plan_raw(off)
        assert st == 0 and st2 == 0 and len(routes) == m
        assert routes == [LANE if n <= D else WAVE if n <= W else BUCKET if n <= B else SINGLE for n in lengths], case
        assert (routes.count(LANE), routes.count(WAVE), routes.count(BUCKET) + routes.count(SINGLE)) == plan[:3], (case, plan)


# ---- the digit recoding, stand-alone under the sanitizers -------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_bucket_digit_recoding_stand_alone_under_asan_ubsan(tmp_path):
    """csrc/segb_digits.h as the kernels use it (tests/host/segb_digits_host.cpp, a program with a main of its own: nothing is loaded into
    python), against Python integers: 32 digits -128 .. 127 with an unsigned top digit 0 .. 128 that recompose s mod 2^255, every one inside
    the 128 buckets, each on the list (bucket, sign) the window kernel files it under; bit 255 reported"""
    L = util.L
    vals = [0, 1, L - 1, L, 2**252 - 1, 2**252 + 1, 2**255 - 1, 2**255, 2**256 - 1, int("80" * 32, 16), int("7f" * 32, 16), 0x7f << 248, 1 << 248,
            127, 128, 129, 255, 256, int("7f" + "80" * 31, 16), int("00" + "7f" * 31, 16)]
    vals += [v << (8 * p) for p in (0, 1, 15, 30, 31) for v in (1, 127, 128, 129, 255) if v << (8 * p) < 2**256]
    rng = np.random.default_rng(54)
    vals += [int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") for _ in range(500)]
    path = tmp_path / "scalars.txt"
    path.write_text("".join(v.to_bytes(32, "little").hex() + "\n" for v in vals))
    exe = str(tmp_path / "segb_digits_host")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                           "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "host", "segb_digits_host.cpp"), "-o", exe])
    env = dict(os.environ); env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=1"; env["UBSAN_OPTIONS"] = "halt_on_error=1"
    r = subprocess.run([exe, str(path)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.endswith("segb_digits_host ok\n"), (r.stdout[-500:], r.stderr[-3000:])
    rows = r.stdout.split("\n")[:-2]
    assert len(rows) == len(vals)
    seen_slots = set()
    for v, row in zip(vals, rows):
        f = [int(x) for x in row.split()]
        top, d, slots = f[0], f[1:33], f[33:]
        low = v % 2**255
        assert top == v >> 255 and len(d) == 32 and len(slots) == 32
        assert sum(x << (8 * k) for k, x in enumerate(d)) == low, hex(v)
        assert all(-128 <= x <= 127 for x in d[:31]) and 0 <= d[31] <= 128, hex(v)
        assert slots == [-1 if x == 0 else 2 * (abs(x) - 1) + (1 if x < 0 else 0) for x in d], hex(v)
        assert all(-1 <= k < 256 for k in slots)
        seen_slots.update(slots)
    assert {0, 1, 254, 255} <= seen_slots                    # both lists of the first and of the last bucket
