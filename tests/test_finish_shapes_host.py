"""tests/pyref_finish.py checked on the host: its restatement of double_and_compress_batch against RFC 9496 ENCODE of 2 P (pyref_h2c), its compress / to_montgomery
against pyref / pyref_montgomery, and the claims tests/test_gpu_finish_shapes.py makes about its sizes and zero-row masks, computed from the launch geometry."""
import random

import numpy as np

import pyref as R
import pyref_finish as F
import pyref_h2c as H
import pyref_montgomery as M

P = F.P


def _points(rng, count):
    return [F.from_affine(*R.ed_mul(rng.randrange(1, 2**40), R.B)) for _ in range(count)]


def test_double_and_compress_is_encode_of_the_double():
    rng = random.Random(1)
    tors = F.torsion8()
    assert len({H.affine(t) for t in tors}) == 8 and all(H.affine(F.double(F.double(F.double(t)))) == (0, 1) for t in tors)
    pts = _points(rng, 24)
    cases = pts + tors + [H.ed_add(p, t) for p in pts[:4] for t in tors]
    for pt in cases:
        for lam in (1, rng.randrange(2, P), P - 1):
            q = F.scale(pt, lam)
            assert F.double_and_compress(q) == H.ristretto_encode(F.double(q)), (pt, lam)
    # 2 T is in E[4] for every T of E[8]: the identity's encoding; e g f h = 0 exactly for E[4] among them
    assert all(F.double_and_compress(t) == bytes(32) for t in tors)
    # a coset P + E[4] doubles to one Ristretto point
    assert len({F.double_and_compress(H.ed_add(pts[0], t)) for t in tors[::2]}) == 1


def test_compress_and_to_montgomery_agree_with_the_other_references():
    rng = random.Random(2)
    for pt in _points(rng, 16) + [(0, 1, 1, 0), (0, P - 1, 1, 0)]:
        q = F.scale(pt, rng.randrange(2, P))
        assert F.compress(q) == R.ed_compress(H.affine(pt)) == H.edwards_compress(q)
        assert F.compress(F.neg(q)) == R.ed_compress(R.ed_neg(H.affine(pt)))
        assert F.to_montgomery(q) == M.to_montgomery(H.affine(pt))
    assert F.to_montgomery((0, 5, 5, 0)) == bytes(32)
    raw = F.to_raw160([q])
    assert F.parse_raw160(raw) == [q]
    from test_gpu_raw160 import relimb
    for cmax in (1, 8191):
        assert F.parse_raw160(relimb(raw, np.random.default_rng(cmax), cmax)) == [q]
    assert all(v * F.scalar_inverse(v) % F.L == 1 for v in (1, 2, F.L - 1, F.L - 2, 2**252))


def test_sizes_reach_every_chain_shape():
    """CH = 16, blocks of 256 lanes: every chain length 1 .. 16, launched lanes without a row, one lane a step longer than the rest at every length, and the
    grid at 256, 512 and 768 lanes with a size on either side of each growth"""
    lens, ragged, idle, grids = set(), set(), False, {}
    for n in F.SIZES:
        ks, out = F.chain_lengths(n)
        lens |= ks
        idle |= out > 0
        if len(ks) == 2 and F.chain_len(n, F.chain_T(n), 1) == min(ks):
            ragged.add(max(ks))                             # lane 0 alone has the extra step
        grids.setdefault(F.chain_T(n), []).append(n)
    assert lens == set(range(1, 17))
    assert ragged == set(range(2, 17))
    assert idle
    assert sorted(grids) == [256, 512, 768]
    assert max(grids[256]) == 4096 and min(grids[512]) == 4097 and max(grids[512]) == 8192 and min(grids[768]) == 8193
    assert all(F.chain_len(n, F.chain_T(n), 0) <= 16 for n in F.SIZES)


def test_masks_reach_every_position_of_a_zero():
    seen = set()
    for name in F.MASKS:
        for n in F.SIZES:
            m = F.zero_mask(name, n, F.chain_T(n))
            assert m.shape == (n,)
            assert np.array_equal(m, F.zero_mask(name, n, F.chain_T(n)))          # seeded
            seen |= F.mask_step_classes(name, n, F.chain_T(n))
    want = {"%s step, %s" % (p, r) for p in ("first", "middle", "last") for r in ("alone", "next to another zero")}
    want |= {"whole chain zero (length 1)", "whole chain zero (length >1)"}
    assert seen == want
    for name, cls in (("middle_step", "middle step, alone"), ("last_step", "last step, alone"), ("two_steps", "middle step, next to another zero"),
                      ("lane3", "whole chain zero (length >1)")):
        assert any(cls in F.mask_step_classes(name, n, F.chain_T(n)) for n in F.SIZES), name
