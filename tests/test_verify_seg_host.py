"""ed25519_verify_batch_segments_plan: the routing of the segmented verify_batch, host arithmetic -- which segments go through the segmented MSM,
which run as single batches, and where the passes are cut.  No GPU."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def pkg():
    import curve25519_dalek_amd as p
    p.load_library()
    return p


def _off(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.uint64))]).astype(np.uint64)


def test_plan_counts(pkg):
    E = pkg.Engine
    seg_max, pass_terms = pkg.engine.VERIFY_SEGMENT_MAX, pkg.engine.MSM_SEGMENT_PASS_TERMS
    assert seg_max == 1023 and 2 * seg_max + 1 <= pkg.engine.MSM_SEGMENT_WAVE_MAX
    # 0, 1, 31, 32, 1023 signatures: 1 + 3 + 63 + 65 + 2047 terms in one pass; 1024 and 5000: single batches
    assert E.verify_batch_segments_plan(_off([0, 1, 31, 32, 1023, 1024, 5000])) == (5, 2, 1, 1 + 3 + 63 + 65 + 2047)
    # a single batch between two runs cuts the pass
    assert E.verify_batch_segments_plan(_off([4, 1024, 4, 0])) == (3, 1, 2, 10)
    assert E.verify_batch_segments_plan(_off([])) == (0, 0, 0, 0)
    assert E.verify_batch_segments_plan(_off([0, 0, 0])) == (3, 0, 1, 3)
    assert E.verify_batch_segments_plan(_off([2000])) == (0, 1, 0, 0)
    assert pass_terms == 1 << 18


def test_plan_rejects_bad_offsets(pkg):
    E = pkg.Engine
    for bad in ([0, 5, 3, 7], [1, 2, 3], [0, 1 << 40]):
        with pytest.raises(pkg.EngineError):
            E.verify_batch_segments_plan(np.array(bad, dtype=np.uint64))
    # m >= 2^32 - 1 is refused before seg_off[m] is read: two readable offsets only
    lib = pkg.load_library()
    two = np.zeros(2, dtype=np.uint64)
    plan = np.zeros(4, dtype=np.uint64)
    for m in (0xffffffff, 1 << 33):
        assert lib.ed25519_verify_batch_segments_plan(two.ctypes.data, C.c_uint64(m), plan.ctypes.data) == -1      # -(hipErrorInvalidValue)
    assert lib.ed25519_verify_batch_segments_plan(None, C.c_uint64(3), plan.ctypes.data) == -1


def test_plan_cuts_tiny_segments_into_passes(pkg):
    E = pkg.Engine
    pt = pkg.engine.MSM_SEGMENT_PASS_TERMS
    # 90 000 segments of one signature: 270 000 terms > 2^18 -> two passes, the first as full as whole segments allow
    segs, seg_long, passes, maxt = E.verify_batch_segments_plan(_off([1] * 90000))
    assert (segs, seg_long) == (90000, 0) and passes == 2 and maxt == (pt // 3) * 3 and maxt <= pt
    # mixed lengths: every pass stays within the limit, and together they hold every term
    rng = np.random.default_rng(11)
    lens = rng.integers(0, 40, size=30000)
    total = int(2 * lens.sum() + lens.shape[0])
    segs, seg_long, passes, maxt = E.verify_batch_segments_plan(_off(lens))
    assert segs == 30000 and seg_long == 0 and maxt <= pt
    assert passes >= 2 and passes >= -(-total // pt) and passes * maxt >= total
    # a longest segment always fits a pass
    assert E.verify_batch_segments_plan(_off([1023] * 200)) == (200, 0, 2, 128 * 2047)
