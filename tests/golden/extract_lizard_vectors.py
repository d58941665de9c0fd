#!/usr/bin/env python3
"""Extract the reference's Lizard known answers into tests/golden/lizard_vectors.json (data only).

Run against a checkout of the reference (its curve25519-dalek/src directory):
    python tests/golden/extract_lizard_vectors.py <curve25519-dalek/src>

  encode              lizard/lizard_ristretto.rs lizard_encode: 4 (16-byte payload, CompressedRistretto) pairs, hex
  sqrt_id_corner      lizard/lizard_ristretto.rs elligator_inv: the input bytes of the fe = +sqrt(i d) corner case, hex
  constants           lizard/u64_constants.rs: SQRT_ID, DP1_OVER_DM1, MDOUBLE_INVSQRT_A_MINUS_D, MIDOUBLE_INVSQRT_A_MINUS_D,
                      MINVSQRT_ONE_PLUS_D as the reference's five radix-2^51 u64 limbs
"""
import json
import os
import re
import sys

REF = None
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ["SQRT_ID", "DP1_OVER_DM1", "MDOUBLE_INVSQRT_A_MINUS_D", "MIDOUBLE_INVSQRT_A_MINUS_D", "MINVSQRT_ONE_PLUS_D"]


def read(rel):
    return open(os.path.join(REF, rel)).read()


def main():
    global REF
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    REF = sys.argv[1]
    lz = read("lizard/lizard_ristretto.rs")
    i = lz.index("fn lizard_encode()")
    body = lz[i:lz.index("for tv in test_vectors", i)]
    pairs = re.findall(r'\(\s*"([0-9a-f]{32})",\s*"([0-9a-f]{64})",?\s*\)', body)
    assert len(pairs) == 4, pairs
    i = lz.index("fn elligator_inv()")
    body = lz[i:lz.index("rng.fill_bytes", i)]
    m = re.search(r"fe_bytes = \[([\s\d,]+)\];", body[body.index("i == 1"):])
    corner = bytes(int(t) for t in re.findall(r"\d+", m.group(1)))
    assert len(corner) == 32
    consts = read("lizard/u64_constants.rs")
    limbs = {}
    for name in NAMES:
        m = re.search(r"pub const " + name + r": FieldElement51 = field_element\(\[([\s\d,]+)\]\);", consts)
        limbs[name] = [int(t) for t in re.findall(r"\d+", m.group(1))]
        assert len(limbs[name]) == 5
    out = {"encode": [list(p) for p in pairs], "sqrt_id_corner": corner.hex(), "constants": limbs}
    with open(os.path.join(HERE, "lizard_vectors.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote lizard_vectors.json: %d encode pairs, %d constants" % (len(pairs), len(limbs)))


if __name__ == "__main__":
    main()
