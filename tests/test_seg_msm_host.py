"""The segmented vartime MSM (csrc/mid_seg.hip) as far as a machine without a GPU can see it: the library exports both entry points, the
engine binds them, dalek exposes the two *_many methods, and the two constants of the header are the engine's and make sense."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("c25519_msm_vartime_segments_dev", "c25519_msm_vartime_segments")


def _header_constant(name):
    hdr = open(os.path.join(ROOT, "include", "c25519_hip.h")).read()
    m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, hdr, flags=re.M)
    assert m, "%s is not defined in include/c25519_hip.h" % name
    return int(m.group(1))


def test_library_exports_both_entry_points():
    import curve25519_dalek_amd as pkg
    lib = pkg.load_library()
    for name in NAMES:
        assert hasattr(lib, name), "libc25519hip.so does not export %s" % name


def test_engine_binds_both_entry_points():
    import ctypes as C
    import curve25519_dalek_amd as pkg
    for name in NAMES:
        assert name in pkg.engine._SIGS and name in pkg.engine.ABI_SYMBOLS
        res, args = pkg.engine._SIGS[name]
        # ctx, scalars, points, n, in_fmt, seg_off, m, out_fmt, out, ok
        assert res is C.c_int32 and len(args) == 10 and args[3] is C.c_uint64 and args[6] is C.c_uint64 and args[4] is C.c_int and args[7] is C.c_int
    assert callable(pkg.Engine.msm_vartime_segments) and callable(pkg.Engine.msm_vartime_segments_t)


def test_dalek_exposes_the_many_forms():
    from curve25519_dalek_amd import dalek
    assert callable(dalek.EdwardsPoint.vartime_multiscalar_mul_many) and callable(dalek.RistrettoPoint.vartime_multiscalar_mul_many)
    assert "vartime_multiscalar_mul_many" in dalek.__doc__


def test_header_constants_are_the_engines_and_sane():
    import curve25519_dalek_amd as pkg
    direct, terms = _header_constant("C25519_MSM_SEGMENT_DIRECT_MAX"), _header_constant("C25519_MSM_SEGMENT_PASS_TERMS")
    assert direct == pkg.engine.MSM_SEGMENT_DIRECT_MAX and terms == pkg.engine.MSM_SEGMENT_PASS_TERMS
    assert 0 < direct < terms
