#!/usr/bin/env python3
"""Extract the reference's MontgomeryPoint test cases into tests/golden/montgomery_vectors.json (data only).

Run against a checkout of the reference (its curve25519-dalek/src directory):
    python tests/golden/extract_montgomery_vectors.py <curve25519-dalek/src>

  x25519_basepoint, ed25519_basepoint      constants.rs X25519_BASEPOINT / ED25519_BASEPOINT_COMPRESSED, hex
  to_edwards                               [u, sign, compressed Edwards point or null]:
      montgomery.rs basepoint_montgomery_to_edwards: u = 9 with sign 0 -> B, sign 1 -> -B (B's x is non-zero, so the
          encoding of -B is that of B with bit 255 set);
      montgomery.rs montgomery_to_edwards_rejects_twist: u = 2 and u = -1 -> null
  eq_defined_mod_p                         montgomery.rs eq_defined_mod_p: the two encodings of u = 18 (18, and 32 bytes of 0xff)
  ladder_matches_edwards                   montgomery.rs montgomery_ladder_matches_edwards_scalarmult on fixed inputs: P = p B and
      s for p, s from SHA-512 of a label, reduced mod l; [u(P), s, u(s P)] with s P computed on the Edwards curve (tests/pyref.py,
      no ladder), as the reference compares s * p_montgomery with (s * p_edwards).to_montgomery()
"""
import hashlib
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pyref as R                               # noqa: E402


def const_bytes(src, name):
    m = re.search(r"pub const " + name + r": \w+ = \w+\(\[([^\]]+)\]\);", src)
    b = bytes(int(t, 16) for t in re.findall(r"0x([0-9a-fA-F]{2})", m.group(1)))
    assert len(b) == 32, name
    return b


def to_montgomery(pt):
    return ((1 + pt[1]) * pow((1 - pt[1]) % R.P, R.P - 2, R.P) % R.P).to_bytes(32, "little")


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    consts = open(os.path.join(ref, "constants.rs")).read()
    mont = open(os.path.join(ref, "montgomery.rs")).read()
    xb, eb = const_bytes(consts, "X25519_BASEPOINT"), const_bytes(consts, "ED25519_BASEPOINT_COMPRESSED")
    neg_eb = eb[:31] + bytes([eb[31] | 0x80])
    # the test bodies the cases come from
    for fn in ("fn basepoint_montgomery_to_edwards()", "fn montgomery_to_edwards_rejects_twist()", "fn eq_defined_mod_p()",
               "fn montgomery_ladder_matches_edwards_scalarmult()"):
        assert fn in mont, fn
    i = mont.index("fn eq_defined_mod_p()")
    body = mont[i:mont.index("assert_eq!", i)]
    u18 = int(re.search(r"u18_bytes\[0\] = (\d+);", body).group(1))
    unred = int(re.search(r"MontgomeryPoint\(\[(\d+); 32\]\)", body).group(1))
    two = (2).to_bytes(32, "little")
    minus_one = (R.P - 1).to_bytes(32, "little")
    to_edwards = [[xb.hex(), 0, eb.hex()], [xb.hex(), 1, neg_eb.hex()], [two.hex(), 0, None], [minus_one.hex(), 0, None]]
    ladder = []
    for j in range(8):
        p = int.from_bytes(hashlib.sha512(b"montgomery ladder point %d" % j).digest(), "little") % R.L
        s = int.from_bytes(hashlib.sha512(b"montgomery ladder scalar %d" % j).digest(), "little") % R.L
        pe = R.ed_mul(p, R.B)
        ladder.append([to_montgomery(pe).hex(), s.to_bytes(32, "little").hex(), to_montgomery(R.ed_mul(s, pe)).hex()])
    out = {"x25519_basepoint": xb.hex(), "ed25519_basepoint": eb.hex(), "to_edwards": to_edwards,
           "eq_defined_mod_p": [bytes([u18] + [0] * 31).hex(), bytes([unred] * 32).hex()], "ladder_matches_edwards": ladder}
    with open(os.path.join(HERE, "montgomery_vectors.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote montgomery_vectors.json: %d to_edwards cases, %d ladder cases" % (len(to_edwards), len(ladder)))


if __name__ == "__main__":
    main()
