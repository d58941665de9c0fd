"""The wave route of the segmented vartime MSM (csrc/mid_seg.hip k_mid_seg_wave) as far as a machine without a GPU can see it: the routing
function c25519_msm_vartime_segments_plan (host arithmetic; the call itself routes with the same code), its binding, the third constant of the
header, and the kernel as compiled for gfx950."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN = "c25519_msm_vartime_segments_plan"
INVALID = -1                                                 # -(hipErrorInvalidValue)


def _header_constant(name):
    hdr = open(os.path.join(ROOT, "include", "c25519_hip.h")).read()
    m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, hdr, flags=re.M)
    assert m, "%s is not defined in include/c25519_hip.h" % name
    return int(m.group(1))


def _consts():
    import curve25519_dalek_amd as pkg
    e = pkg.engine
    return e.MSM_SEGMENT_DIRECT_MAX, e.MSM_SEGMENT_WAVE_MAX, e.MSM_SEGMENT_PASS_TERMS


def _plan_raw(off, m=None):
    """-> (status, plan) of the C function on the offsets as given (no checks on this side)"""
    import curve25519_dalek_amd as pkg
    lib = pkg.load_library()
    off = np.ascontiguousarray(np.asarray(off, dtype=np.uint64))
    plan = np.full(5, 0xEE, np.uint64)
    st = getattr(lib, PLAN)(off.ctypes.data if off.size else None, len(off) - 1 if m is None else m, plan.ctypes.data)
    return st, tuple(int(x) for x in plan)


def _off(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.uint64))]).astype(np.uint64)


def _model(lengths, D, W, T):
    """the routing rule of the header, restated: by length alone; a pass is a run of lane and wave segments of at most T terms, cut only by that
    count and by the single-MSM segments"""
    lane = wave = single = passes = most = 0
    segs = terms = 0
    for n in lengths:
        if n > W:
            single += 1
            if segs:
                passes += 1; most = max(most, terms)
            segs = terms = 0
            continue
        if terms + n > T:
            if segs:
                passes += 1; most = max(most, terms)
            segs = terms = 0
        segs += 1; terms += n
        if n > D:
            wave += 1
        else:
            lane += 1
    if segs:
        passes += 1; most = max(most, terms)
    return lane, wave, single, passes, most


# ---- export and binding ---------------------------------------------------------------------------------------------------------
def test_library_exports_the_plan_function():
    import curve25519_dalek_amd as pkg
    assert hasattr(pkg.load_library(), PLAN), "libc25519hip.so does not export %s" % PLAN


def test_engine_binds_the_plan_function():
    import curve25519_dalek_amd as pkg
    assert PLAN in pkg.engine._SIGS and PLAN in pkg.engine.ABI_SYMBOLS
    res, args = pkg.engine._SIGS[PLAN]
    assert res is C.c_int32 and len(args) == 3 and args[1] is C.c_uint64      # seg_off, m, plan
    assert callable(pkg.Engine.msm_vartime_segments_plan)


def test_wave_constant_is_the_engines_and_lies_between_the_other_two():
    D, W, T = _consts()
    assert _header_constant("C25519_MSM_SEGMENT_WAVE_MAX") == W
    assert _header_constant("C25519_MSM_SEGMENT_DIRECT_MAX") == D and _header_constant("C25519_MSM_SEGMENT_PASS_TERMS") == T
    assert D < W <= T


# ---- the plan on hand-made offsets ----------------------------------------------------------------------------------------------
def test_plan_routes_by_length():
    D, W, T = _consts()
    lengths = [0, 1, D, D + 1, W, W + 1]
    st, plan = _plan_raw(_off(lengths))
    assert st == 0 and plan == (3, 2, 1, 1, 1 + D + D + 1 + W)
    assert plan == _model(lengths, D, W, T)


def test_a_single_msm_segment_in_the_middle_cuts_the_passes():
    D, W, T = _consts()
    lengths = [3, D + 5, 2, W + 1, 7, D + 1]
    st, plan = _plan_raw(_off(lengths))
    assert st == 0 and plan == (3, 2, 1, 2, max(3 + D + 5 + 2, 7 + D + 1))
    st, plan = _plan_raw(_off([W + 1, W + 2]))              # nothing but single-MSM segments: no pass at all
    assert st == 0 and plan == (0, 0, 2, 0, 0)


def test_wave_segments_beyond_the_pass_size_make_two_passes():
    D, W, T = _consts()
    k = T // W + 1                                           # k segments of W terms: just over T terms in all
    lengths = [W] * k
    assert T < sum(lengths) <= T + W
    st, plan = _plan_raw(_off(lengths))
    assert st == 0 and plan[:4] == (0, k, 0, 2) and plan[4] <= T
    assert plan == _model(lengths, D, W, T)


def test_plan_degenerate_and_rejected_offsets():
    D, W, T = _consts()
    assert _plan_raw([0], 0) == (0, (0, 0, 0, 0, 0))        # m = 0
    assert _plan_raw([], 0) == (0, (0, 0, 0, 0, 0))         # ... where seg_off may be null, as in the call
    assert _plan_raw([0, 0, 0]) == (0, (2, 0, 0, 1, 0))     # empty segments are lane segments (they give the identity)
    # the call's validation and the call's error.  The function is not given n: it takes seg_off[m] for it, so "does not end at n" has no
    # counterpart here beyond the call's bound on n itself
    for bad in ([1, 2, 4], [0, 3, 2, 4], [0, 2, 1], [0, 5, 1 << 40]):
        st, _ = _plan_raw(bad)
        assert st == INVALID, (bad, st)
    st, _ = _plan_raw([], 3)                                 # null offsets with m > 0
    assert st == INVALID


def test_engine_method_needs_no_gpu_and_raises_on_bad_offsets():
    import curve25519_dalek_amd as pkg
    D, W, T = _consts()
    assert pkg.Engine.msm_vartime_segments_plan([0, 1, 1 + D, 2 + 2 * D, 3 + 2 * D + W]) == (2, 1, 1, 1, 2 + 2 * D)
    with pytest.raises(pkg.engine.EngineError):
        pkg.Engine.msm_vartime_segments_plan([0, 3, 2])


# ---- random offsets -------------------------------------------------------------------------------------------------------------
def test_plan_agrees_with_the_rule_on_random_offsets():
    D, W, T = _consts()
    rng = np.random.default_rng(31)
    edges = [0, 1, D - 1, D, D + 1, W - 1, W, W + 1, 2 * W]
    for case in range(200):
        m = int(rng.integers(1, 400))
        kind = case % 4
        if kind == 0:                                        # short segments
            lengths = rng.integers(0, 2 * D, size=m)
        elif kind == 1:                                      # the boundaries themselves
            lengths = rng.choice(edges, size=m)
        elif kind == 2:                                      # wave segments that fill passes, a few single-MSM ones among them
            lengths = np.where(rng.random(m) < 0.05, W + 1 + rng.integers(0, 100, size=m), rng.integers(W // 2, W + 1, size=m))
        else:
            lengths = np.where(rng.random(m) < 0.5, rng.integers(0, D + 1, size=m), rng.integers(D + 1, 3 * W // 2, size=m))
        lengths = [int(x) for x in lengths]
        st, plan = _plan_raw(_off(lengths))
        assert st == 0 and plan[0] + plan[1] + plan[2] == m, (case, plan)
        assert plan == _model(lengths, D, W, T), (case, plan)
        assert plan[4] <= T


# ---- the kernel as compiled -----------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(util.HIPCC), reason="hipcc not available")
def test_wave_kernel_as_compiled(tmp_path_factory):
    kernels = util.asm_kernels(util.device_asm(tmp_path_factory, "mid_seg"))
    named = {util.demangle_kernel(sym): v for sym, v in kernels.items()}
    wave = [k for k in named if k and k.startswith("k_mid_seg_wave")]
    assert len(wave) == 1 and re.fullmatch(r"k_mid_\w+(<\d>)?", wave[0]), sorted(named)
    body, priv = named[wave[0]]
    assert priv == 0, "k_mid_seg_wave spills: private segment of %d bytes" % priv
    ops = util.asm_ops(body)
    assert any(o.startswith(("ds_bpermute", "v_permlane", "v_readlane")) or "_dpp" in o for o in ops), "no cross-lane move in k_mid_seg_wave"
    assert any(o.startswith("v_mad_u64_u32") for o in ops), "no 32 x 32 -> 64 multiply in k_mid_seg_wave"
