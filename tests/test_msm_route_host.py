"""Which path serves a call (csrc/msm.hip "routes"), as far as a machine without a GPU can see it: c25519_msm_route -- host arithmetic, the call itself
routes with the same code -- through its binding Engine.msm_route, on both sides of every boundary of the table in DESIGN.md "which path serves a call"."""
import ctypes as C
import subprocess

import pytest

import util

ROUTE = "c25519_msm_route"
EDWARDS_Y, RISTRETTO, RAW = 0, 1, 2


def route(kind, n, in_fmt=RAW, host=False):
    import curve25519_dalek_amd as pkg
    return pkg.Engine.msm_route(kind, n, in_fmt, host)


def geometry_c(n):
    import curve25519_dalek_amd as pkg
    c, nwin = C.c_int32(0), C.c_int32(0)
    pos, wid, addk = (C.c_uint8 * 56)(), (C.c_uint8 * 56)(), (C.c_uint32 * 8)()
    assert pkg.load_library().c25519_msm_geometry(n, C.byref(c), C.byref(nwin), pos, wid, addk) == 0
    return c.value


def test_export_and_binding():
    import curve25519_dalek_amd as pkg
    assert hasattr(pkg.load_library(), ROUTE), "libc25519hip.so does not export %s" % ROUTE
    assert ROUTE in pkg.engine._SIGS and ROUTE in pkg.engine.ABI_SYMBOLS
    res, args = pkg.engine._SIGS[ROUTE]
    assert res is C.c_int32 and len(args) == 5 and args[1] is C.c_uint64      # kind, n, in_fmt, host_pointers, route
    for bad in ((2, 5, RAW), (-1, 5, RAW), (0, 5, 3), (0, 1 << 40, RAW), (1, 1 << 40, RAW)):
        with pytest.raises(pkg.engine.EngineError):
            pkg.Engine.msm_route(*bad)
    for kind in (0, 1):
        r = route(kind, 0)
        assert r["path"] == "empty" and r["passes"] == 0 and not r["publish"]


# (n, path, width, passes, publishes itself) -- raw points, device pointers, two stream sets
RAW_ROWS = [
    (1, "small", 5, 1, True), (1023, "small", 5, 1, True),
    (1024, "small", 6, 1, True), (4095, "small", 6, 1, True), (4096, "small", 6, 1, True), (6143, "small", 6, 1, True),
    (6144, "mid", 12, 1, True), (8191, "mid", 12, 1, True),
    (8192, "mid", 13, 1, True), (16383, "mid", 13, 1, True), (16384, "mid", 13, 1, True), (32767, "mid", 13, 1, True),
    (32768, "mid", 14, 1, True), (65535, "mid", 14, 1, True),
    (65536, "mid", 15, 1, True), (131072, "mid", 15, 1, True), (1 << 18, "mid", 15, 1, True),
    ((1 << 18) + 1, "pipeline", 15, 1, False), ((1 << 18) + 2, "pipeline", 15, 1, False), ((1 << 19), "pipeline", 16, 1, False),
    ((1 << 20), "pipeline", 16, 1, False), ((1 << 21), "pipeline", 17, 1, False), (2625000, "pipeline", 17, 1, False),
    (2625001, "pipeline", 16, 2, False), (3500001, "pipeline", 17, 3, False), (1 << 24, "pipeline", 17, 10, False),
]


@pytest.mark.parametrize("n,path,c,passes,publish", RAW_ROWS)
def test_raw_points_device(n, path, c, passes, publish):
    r = route(0, n)
    assert (r["path"], r["c"], r["passes"], r["publish"]) == (path, c, passes, publish), r
    assert not r["prep_points"]
    assert r["per"] == -(-n // passes)
    # the width is the one c25519_msm_geometry reports for the terms the layout is derived from: n itself for a single pass
    assert r["layout_terms"] == n if passes == 1 else r["layout_terms"] >= r["per"]
    assert r["c"] == geometry_c(r["layout_terms"])


def test_layout_of_several_passes():
    assert route(0, 2625001)["layout_terms"] == 1312501                  # two passes on two stream sets: the layout of a pass
    assert route(0, 3500001)["layout_terms"] == 1 << 21                  # more passes than stream sets: from 2^21 terms
    r = route(0, 1 << 24)
    assert r["per"] == -(-(1 << 24) // 10) and r["layout_terms"] == 1 << 21


@pytest.mark.parametrize("fmt", [EDWARDS_Y, RISTRETTO])
def test_encoded_points_device(fmt):
    for n, path, c in [(1, "small", 5), (1023, "small", 5), (1024, "small", 6), (4095, "small", 6),
                       (4096, "mid", 12), (6143, "mid", 12), (6144, "mid", 12), (8191, "mid", 12),
                       (8192, "mid", 13), (1 << 18, "mid", 15), ((1 << 18) + 1, "mid", 15),
                       ((1 << 18) + 2, "pipeline", 15), (2625000, "pipeline", 17)]:
        r = route(0, n, fmt)
        assert (r["path"], r["c"], r["passes"]) == (path, c, 1), (n, r)
        assert r["prep_points"] and not r["publish"], (n, r)             # records first; an encoded call never publishes its record itself
        if n > 6143:
            assert r["c"] == route(0, n)["c"]                            # "as raw"
    r = route(0, 2625001, fmt)
    assert (r["path"], r["c"], r["passes"]) == ("pipeline", 16, 2)


def test_host_pointers_take_the_same_paths():
    for fmt in (RAW, EDWARDS_Y):
        for n in (1, 1023, 1024, 4095, 4096, 6143, 6144, 8191, 8192, 1 << 18, (1 << 18) + 1, (1 << 18) + 2, (1 << 20) - 1):
            d, h = route(0, n, fmt), route(0, n, fmt, True)
            assert (h["path"], h["c"], h["passes"], h["prep_points"]) == (d["path"], d["c"], d["passes"], d["prep_points"]), (fmt, n, h)
            assert h["publish"] == d["publish"], (fmt, n, h)             # (a small host-pointer call goes up in one staged copy: no fetch)
    # from 2^20 terms the inputs go up in passes of 2^19 terms (raw) / 2^20 terms (encoded)
    r = route(0, 1 << 20, RAW, True)
    assert (r["path"], r["passes"], r["per"]) == ("pipeline", 2, 1 << 19)
    r = route(0, (3 << 18) + (1 << 20), RAW, True)
    assert (r["passes"], r["per"]) == (4, -(-((3 << 18) + (1 << 20)) // 4))
    r = route(0, 1 << 20, EDWARDS_Y, True)
    assert (r["path"], r["passes"], r["per"]) == ("pipeline", 1, 1 << 20)
    r = route(0, (3 << 19) + 1, EDWARDS_Y, True)
    assert (r["passes"], r["per"]) == (2, (3 << 18) + 1) and route(0, (3 << 19) + 1, EDWARDS_Y)["passes"] == 1


# (signatures, path, width or None, published from the hash chain's stream)
VERIFY_ROWS = [
    (1, "small", None, False), (2047, "small", None, False),
    (2048, "mid", 12, True), (4095, "mid", 12, True),
    (4096, "mid", 13, True), (12287, "mid", 13, True),
    (12288, "mid", 14, True), (49151, "mid", 14, True),
    (49152, "mid", 16, True), (65536, "mid", 16, True),
    (65537, "mid", 16, False), (131072, "mid", 16, False),
    (131073, "pipeline", None, False), (1 << 20, "pipeline", 16, False),
]


@pytest.mark.parametrize("n,path,c,chain", VERIFY_ROWS)
def test_verify_batch_device(n, path, c, chain):
    r = route(1, n)
    assert r["path"] == path and r["passes"] == 1 and r["per"] == n and r["layout_terms"] == 2 * n + 1, r
    assert c is None or r["c"] == c, r
    assert r["c"] <= 16                                                  # the cap of a batch's layout
    assert r["publish"] == chain, r


def test_verify_batch_passes_and_host_pointers():
    r = route(1, (3 << 19) + 1)                                          # beyond 1.5 x 2^20 signatures: two independent passes
    assert (r["path"], r["passes"], r["per"], r["layout_terms"]) == ("pipeline", 2, (3 << 18) + 1, (3 << 19) + 3) and r["c"] <= 16
    # (at most 128 signatures through host pointers: verify_batch_small_host, outside this export -- tests/test_gpu_msm_route.py checks it on the GPU)
    for n in (129, 2047, 2048, 16384):                                   # one staged copy up, then as on the device
        assert route(1, n, host=True) == route(1, n)
    r = route(1, 16385, host=True)                                       # the arrays go up pass by pass: the mid path, off the chain, record copied
    assert (r["path"], r["c"], r["publish"]) == ("mid", 14, False) and route(1, 16385)["publish"]


CHILD = r'''
import curve25519_dalek_amd as pkg
a, b = pkg.Engine.msm_route(0, 98304), pkg.Engine.msm_route(0, 98305)
assert (a["path"], a["passes"], a["c"]) == ("mid", 1, 15), a
assert (b["path"], b["passes"], b["per"], b["publish"]) == ("pipeline", 2, 49153, False), b
print("child route ok")
'''


def test_pass_size_knob_of_the_tuning_build_moves_the_split():
    """C25519_MSM_PASS_LOG2 = 16: a pass holds at most 1.5 x 2^16 terms -- 98304 terms are one pass on the mid path, 98305 two passes on the bucket pipeline"""
    out = subprocess.run(util.child_argv(CHILD), capture_output=True, text=True, timeout=300, env=util.tune_env({"C25519_MSM_PASS_LOG2": "16"}))
    assert out.returncode == 0 and "child route ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert route(0, 98305)["passes"] == 1                                # (the release library in this process reads no environment)
