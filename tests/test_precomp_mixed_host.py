"""Many mixed multiscalar muls over one precomputed point set (csrc/mid_mixed.hip) as far as a machine without a GPU can see them: the three
exported symbols and their bindings, the front-end methods, the planning function c25519_precomp_msm_vartime_mixed_rows_plan (host
arithmetic; the call validates, routes and cuts its passes with the same code) against a restatement of the rule built from the header's
constants, and the wave kernel as compiled for gfx950."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("c25519_precomp_msm_vartime_mixed_rows_dev", "c25519_precomp_msm_vartime_mixed_rows", "c25519_precomp_msm_vartime_mixed_rows_plan")
PLAN = SYMS[2]
INVALID = -1                                                 # -(hipErrorInvalidValue)
NAMES = ("C25519_PRECOMP_ROWS_LANE", "C25519_PRECOMP_ROWS_WAVE", "C25519_PRECOMP_ROWS_LANE_WIDTH", "C25519_PRECOMP_ROWS_LANE_MIN_ROWS",
         "C25519_PRECOMP_MIXED_LANE_DYN_MAX", "C25519_PRECOMP_MIXED_LANE_BASE_ROWS", "C25519_PRECOMP_MIXED_LANE_ROWS_PER_TERM",
         "C25519_MSM_SEGMENT_DIRECT_MAX", "C25519_MSM_SEGMENT_WAVE_MAX", "C25519_MSM_SEGMENT_PASS_TERMS")


def _header_constant(name):
    hdr = open(os.path.join(ROOT, "include", "c25519_hip.h")).read()
    m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, hdr, flags=re.M)
    assert m, "%s is not defined in include/c25519_hip.h" % name
    return int(m.group(1))


@pytest.fixture(scope="module")
def hdr():
    return {n.split("_", 1)[1]: _header_constant(n) for n in NAMES}


def _off(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.uint64))]).astype(np.uint64)


def _plan_raw(m, w, off):
    """-> (status, plan) of the C function on the arguments as given (no checks on this side); off: a sequence, or None for a null pointer"""
    import curve25519_dalek_amd as pkg
    plan = np.full(4, 0xEE, np.uint64)
    if off is not None:
        off = np.ascontiguousarray(np.asarray(off, dtype=np.uint64))
    st = getattr(pkg.load_library(), PLAN)(m, w, off.ctypes.data if off is not None and off.size else None, plan.ctypes.data)
    return st, tuple(int(x) for x in plan)


def _lane_rows(w, longest, h):
    """the fewest rows from which AUTO takes the lane route, None if it never does"""
    if w >= h["PRECOMP_ROWS_LANE_WIDTH"]:
        return None
    if longest == 0:                                         # no dynamic term anywhere: the rows call, and its rule
        return h["PRECOMP_ROWS_LANE_MIN_ROWS"]
    if longest > h["PRECOMP_MIXED_LANE_DYN_MAX"]:
        return None
    return h["PRECOMP_MIXED_LANE_BASE_ROWS"] + h["PRECOMP_MIXED_LANE_ROWS_PER_TERM"] * (w + longest)


def _model(w, lengths, h):
    """the rule of the header, restated.  Route, with t = w + the dynamic terms of the longest row: wave for w >= LANE_WIDTH; the rows call's
    rule (lane iff m >= LANE_MIN_ROWS) if no row has a dynamic term; else lane iff the longest row has at most MIXED_LANE_DYN_MAX dynamic
    terms and m >= MIXED_LANE_BASE_ROWS + MIXED_LANE_ROWS_PER_TERM * t.  A pass is a run of consecutive rows of at most PASS_TERMS dynamic
    terms in all; a wave of the lane route carries 64 consecutive rows of one pass, a wave of the wave route one row"""
    m = len(lengths)
    need = _lane_rows(w, max(lengths, default=0), h)
    lane = need is not None and m >= need
    passes, most, lane_waves, rows, terms = 0, 0, 0, 0, 0
    for n in lengths:
        if terms + n > h["MSM_SEGMENT_PASS_TERMS"]:
            passes += 1; most = max(most, terms); lane_waves += (rows + 63) // 64
            rows = terms = 0
        rows += 1; terms += n
    if rows:
        passes += 1; most = max(most, terms); lane_waves += (rows + 63) // 64
    return (h["PRECOMP_ROWS_LANE"], lane_waves, passes, most) if lane else (h["PRECOMP_ROWS_WAVE"], m, passes, most)


# ---- exports, bindings, front ends ------------------------------------------------------------------------------------------------
def test_library_exports_the_three_symbols():
    import curve25519_dalek_amd as pkg
    lib = pkg.load_library()
    assert [s for s in SYMS if not hasattr(lib, s)] == []


def test_engine_binds_the_three_symbols():
    import curve25519_dalek_amd as pkg
    sigs = pkg.engine._SIGS
    assert [s for s in SYMS if s not in sigs or s not in pkg.engine.ABI_SYMBOLS] == []
    for name in SYMS[:2]:   # ctx, handle, static scalars, m, w, dyn scalars, dyn points, n_dyn, in_fmt, dyn_off, route, out_fmt, out, ok
        res, args = sigs[name]
        assert res is C.c_int32 and len(args) == 14, name
        assert [i for i, a in enumerate(args) if a is C.c_uint64] == [3, 4, 7], name
        assert args[8] is C.c_int and args[10] is C.c_int32 and args[11] is C.c_int, name
        assert all(args[i] is C.c_void_p for i in (0, 1, 2, 5, 6, 9, 12, 13)), name
    res, args = sigs[PLAN]                                   # m, w, dyn_off, plan
    assert res is C.c_int32 and args == [C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]


def test_front_end_methods_exist():
    import curve25519_dalek_amd as pkg
    from curve25519_dalek_amd import dalek
    for name in ("precomp_msm_vartime_mixed_rows", "precomp_msm_vartime_mixed_rows_t", "precomp_msm_vartime_mixed_rows_plan"):
        assert callable(getattr(pkg.Engine, name, None)), name
    for cls in (dalek.VartimeEdwardsPrecomputation, dalek.VartimeRistrettoPrecomputation):
        assert callable(getattr(cls, "vartime_mixed_multiscalar_mul_many", None)), cls.__name__
    assert "vartime_mixed_multiscalar_mul_many" in dalek.__doc__


def test_header_constants_are_the_engines(hdr):
    import curve25519_dalek_amd as pkg
    assert {n: getattr(pkg.engine, n) for n in hdr} == hdr
    assert hdr["MSM_SEGMENT_DIRECT_MAX"] < hdr["MSM_SEGMENT_WAVE_MAX"] <= hdr["MSM_SEGMENT_PASS_TERMS"]


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
def test_plan_obeys_the_headers_constants_on_a_grid(hdr):
    W, R = hdr["PRECOMP_ROWS_LANE_WIDTH"], hdr["PRECOMP_ROWS_LANE_MIN_ROWS"]
    D, X, K = hdr["MSM_SEGMENT_DIRECT_MAX"], hdr["MSM_SEGMENT_WAVE_MAX"], hdr["PRECOMP_MIXED_LANE_DYN_MAX"]
    L, V = hdr["PRECOMP_ROWS_LANE"], hdr["PRECOMP_ROWS_WAVE"]
    seen = set()
    for w in (0, 1, W - 1, W, W + 1, 4096):
        for longest in (0, 1, K - 1, K, K + 1, D, D + 1, X):
            need = _lane_rows(w, longest, hdr)
            ms = {1, 64, 65, R - 1, R, R + 1} | ({need - 1, need, need + 1} if need else set())
            for m in sorted(x for x in ms if x >= 1):
                for where in {0, m - 1}:                     # the longest row first or last; every other row has min(1, longest) dynamic terms
                    lengths = [min(1, longest)] * m
                    lengths[where] = longest
                    st, plan = _plan_raw(m, w, _off(lengths))
                    assert st == 0 and plan == _model(w, lengths, hdr), (m, w, longest, where, st, plan)
                    assert (plan[0] == L) == (need is not None and m >= need), (m, w, longest)
                    seen.add((plan[0], w < W, longest == 0, longest <= K, need is not None and m >= need))
    # both routes occur on either side of every constant: the width, the longest row, the row count (with and without dynamic terms)
    assert {(L, True, True, True, True), (V, True, True, True, False), (L, True, False, True, True), (V, True, False, True, False),
            (V, True, False, False, False), (V, False, False, True, False), (V, False, True, True, False)} <= seen
    assert _lane_rows(2, 1, hdr) < R                         # with a dynamic term the lanes win from fewer rows than in the rows call


def test_plan_cuts_passes_at_row_boundaries(hdr):
    X, T = hdr["MSM_SEGMENT_WAVE_MAX"], hdr["MSM_SEGMENT_PASS_TERMS"]
    k = T // X + 1                                           # k rows of X dynamic terms: just over T in all
    lengths = [X] * k
    st, plan = _plan_raw(k, 2, _off(lengths))
    assert st == 0 and plan == _model(2, lengths, hdr) and plan[2] == 2 and plan[3] <= T
    lengths = [0] * 100 + [X] * (T // X) + [0, 0, 1] + [0] * 70       # rows without dynamic terms stay in the pass that is open
    st, plan = _plan_raw(len(lengths), 0, _off(lengths))
    assert st == 0 and plan == _model(0, lengths, hdr) and plan[2:] == (2, T)
    assert _plan_raw(3, 5, [0, 0, 0, 0]) == (0, (hdr["PRECOMP_ROWS_WAVE"], 3, 1, 0))
    assert _plan_raw(0, 5, [0]) == (0, (hdr["PRECOMP_ROWS_WAVE"], 0, 0, 0))
    assert _plan_raw(0, 5, None) == (0, (hdr["PRECOMP_ROWS_WAVE"], 0, 0, 0))      # m = 0: dyn_off may be null, as in the call


def test_plan_agrees_with_the_rule_on_random_offsets(hdr):
    W, R = hdr["PRECOMP_ROWS_LANE_WIDTH"], hdr["PRECOMP_ROWS_LANE_MIN_ROWS"]
    D, X, T, K = hdr["MSM_SEGMENT_DIRECT_MAX"], hdr["MSM_SEGMENT_WAVE_MAX"], hdr["MSM_SEGMENT_PASS_TERMS"], hdr["PRECOMP_MIXED_LANE_DYN_MAX"]
    rng = np.random.default_rng(59)
    edges = [0, 1, D - 1, D, D + 1, X - 1, X]
    for case in range(200):
        kind = case % 4
        m = int(rng.integers(1, 400))
        w = int(rng.choice([0, 1, 2, W - 1, W, W + 1, 130]))
        if kind == 0:                                        # short rows, as many as the lane route needs, a few more or a few less
            longest = int(rng.integers(0, K + 2))
            need = _lane_rows(w, longest, hdr)
            m = max(1, (need or R) + int(rng.integers(-3, 4)))
            lengths = rng.integers(0, longest + 1, size=m)
            lengths[int(rng.integers(0, m))] = longest
        elif kind == 1:                                      # the boundaries themselves
            lengths = rng.choice(edges, size=m)
        elif kind == 2:                                      # long rows that fill passes
            lengths = rng.integers(X // 2, X + 1, size=m)
        else:
            lengths = np.where(rng.random(m) < 0.5, rng.integers(0, D + 1, size=m), rng.integers(D + 1, X + 1, size=m))
        lengths = [int(x) for x in lengths]
        st, plan = _plan_raw(m, w, _off(lengths))
        assert st == 0 and plan == _model(w, lengths, hdr), (case, m, w, st, plan)
        assert plan[3] <= T and plan[2] >= 1


def test_plan_refuses_what_the_call_refuses(hdr):
    X = hdr["MSM_SEGMENT_WAVE_MAX"]
    assert _plan_raw(3, 2, [0, 1, 1, 4])[0] == 0
    for bad in ([1, 2, 4, 4], [0, 3, 2, 4], [0, 2, 2, 1]):   # does not start at 0; decreases
        assert _plan_raw(3, 2, bad)[0] == INVALID, bad
    assert _plan_raw(3, 2, None)[0] == INVALID               # null offsets with m > 0
    assert _plan_raw(2, 2, [0, X, 2 * X])[0] == 0
    assert _plan_raw(2, 2, [0, X + 1, X + 2])[0] == INVALID and _plan_raw(2, 2, [0, 1, X + 2])[0] == INVALID      # a row of WAVE_MAX + 1 terms
    assert _plan_raw(2, 2, [0, 5, 1 << 40])[0] == INVALID
    # m >= 2^32 - 1 is refused before dyn_off[m] is read: a one-element array (and a null pointer) would otherwise be read far out of bounds
    for m in ((1 << 32) - 1, 1 << 32, (1 << 64) - 1):
        assert _plan_raw(m, 1, [0])[0] == INVALID and _plan_raw(m, 0, None)[0] == INVALID, m
    assert _plan_raw(3, (1 << 64) - 1, [0, 0, 0, 0])[0] == INVALID        # m * w overflows
    assert _plan_raw(1, (1 << 64) - 1, [0, 0])[0] == 0


def test_engine_plan_needs_no_gpu_and_raises_on_a_refused_shape(hdr):
    import curve25519_dalek_amd as pkg
    D, X = hdr["MSM_SEGMENT_DIRECT_MAX"], hdr["MSM_SEGMENT_WAVE_MAX"]
    assert pkg.Engine.precomp_msm_vartime_mixed_rows_plan(3, 130, [0, 17, 34, 51]) == (hdr["PRECOMP_ROWS_WAVE"], 3, 1, 51)
    R = hdr["PRECOMP_ROWS_LANE_MIN_ROWS"]
    assert pkg.Engine.precomp_msm_vartime_mixed_rows_plan(R, 2, np.arange(R + 1)) == (hdr["PRECOMP_ROWS_LANE"], (R + 63) // 64, 1, R)
    assert pkg.Engine.precomp_msm_vartime_mixed_rows_plan(R, 2, _off([1] * (R - 1) + [D + 1]))[0] == hdr["PRECOMP_ROWS_WAVE"]
    assert pkg.Engine.precomp_msm_vartime_mixed_rows_plan(R - 1, 2, [0] * R)[0] == hdr["PRECOMP_ROWS_WAVE"]        # no dynamic term: the rows call's rule
    assert pkg.Engine.precomp_msm_vartime_mixed_rows_plan(R, 2, [0] * (R + 1))[0] == hdr["PRECOMP_ROWS_LANE"]
    assert pkg.Engine.precomp_msm_vartime_mixed_rows_plan(0, 2, [0]) == (hdr["PRECOMP_ROWS_WAVE"], 0, 0, 0)
    for bad in ([0, 3, 2], [0, 1, X + 2]):
        with pytest.raises(pkg.engine.EngineError):
            pkg.Engine.precomp_msm_vartime_mixed_rows_plan(2, 2, bad)


# ---- the kernels as compiled ------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(util.HIPCC), reason="hipcc not available")
def test_mixed_kernels_as_compiled(tmp_path_factory):
    kernels = util.asm_kernels(util.device_asm(tmp_path_factory, "mid_mixed"))
    named = {util.demangle_kernel(sym): v for sym, v in kernels.items()}
    assert all(k and re.fullmatch(r"k_mid_\w+(<\d>)?", k) for k in named), sorted(map(str, named))
    assert not [k for k in named if k.startswith(("k_mid_seg_wave", "k_mid_vseg_transcript"))]
    assert {"k_mid_mixed_lane", "k_mid_mixed_wave"} == set(named), sorted(named)
    for k in ("k_mid_mixed_lane", "k_mid_mixed_wave"):
        body, priv = named[k]
        assert priv == 0, "%s spills: private segment of %d bytes" % (k, priv)
        assert any(o.startswith("v_mad_u64_u32") for o in util.asm_ops(body)), "no 32 x 32 -> 64 multiply in %s" % k
    ops = util.asm_ops(named["k_mid_mixed_wave"][0])
    assert any(o.startswith(("ds_bpermute", "v_permlane", "v_readlane")) or "_dpp" in o for o in ops), "no cross-lane move in k_mid_mixed_wave"
