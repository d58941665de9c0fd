#!/usr/bin/env python3
"""Extract the reference's hash-to-group known answers into tests/golden/h2c_vectors.json (data only).

Run in the build container (reads /root/reference, which does NOT exist on the GPU box):
    python tests/golden/extract_h2c_vectors.py

  elligator_sage      ristretto/elligator.rs elligator_vs_ristretto_sage: 16 (r_0 bytes, CompressedRistretto) pairs
  one_way_map         ristretto/elligator.rs one_way_map: (64 uniform bytes, CompressedRistretto) -- RFC 9496 A.3
  hash_to_curve       edwards.rs RFC_HASH_TO_CURVE_KAT (RFC 9380 J.5.1) with its DST: (msg, x, y), x / y big-endian hex
  encode_to_curve     edwards.rs RFC_ENCODE_TO_CURVE_KAT (RFC 9380 J.5.2) with its DST
  hash_to_field_1/_2  field.rs RFC_HASH_TO_FIELD_KAT / _KAT_2 with their DSTs: (msg, u0[, u1]), big-endian hex
Messages are stored as hex.
"""
import json
import os
import re

REF = "/root/reference/curve25519-dalek/src"
HERE = os.path.dirname(os.path.abspath(__file__))


def read(rel):
    return open(os.path.join(REF, rel)).read()


def rust_bytes_lit(s):
    """the body of a Rust b"..." literal: `\\` + newline + leading whitespace is a line continuation"""
    s = re.sub(r"\\\n\s*", "", s)
    assert "\\" not in s
    return s.encode()


def byte_arrays(text):
    return [bytes(int(t, 0) for t in re.findall(r"0x[0-9a-fA-F]+|\d+", m)) for m in re.findall(r"\[([\s\d,xa-fA-F]+)\]", text)]


def section(text, start, end):
    i = text.index(start)
    return text[i:text.index(end, i)]


def kat_tuples(text, name, nhex):
    body = section(text, "const " + name + ":", "];")
    pat = r'\(\s*b"((?:[^"\\]|\\\n)*)",' + r'\s*"([0-9a-f]{64})",?' * nhex + r"\s*\)"
    out = []
    for m in re.finditer(pat, body):
        out.append([rust_bytes_lit(m.group(1)).hex()] + [m.group(2 + k) for k in range(nhex)])
    return out


def main():
    ell = read("ristretto/elligator.rs")
    sage = section(ell, "fn elligator_vs_ristretto_sage", "for i in 0..16")
    ins = byte_arrays(section(sage, "let bytes", "let encoded_images"))
    outs = byte_arrays(section(sage, "let encoded_images", "];"))
    assert len(ins) == 16 and len(outs) == 16 and all(len(x) == 32 for x in ins + outs)
    owm = byte_arrays(section(ell, "fn one_way_map", "for (input, output)"))
    owm = [a for a in owm if len(a) in (32, 64)]
    assert len(owm) % 2 == 0 and all(len(owm[2 * i]) == 64 and len(owm[2 * i + 1]) == 32 for i in range(len(owm) // 2))

    ed = read("edwards.rs")
    fld = read("field.rs")
    dst_nu = "QUUX-V01-CS02-with-edwards25519_XMD:SHA-512_ELL2_NU_"
    dst_ro = "QUUX-V01-CS02-with-edwards25519_XMD:SHA-512_ELL2_RO_"
    assert dst_nu in ed and dst_ro in ed and dst_nu in fld and dst_ro in fld
    data = {
        "elligator_sage": [[a.hex(), b.hex()] for a, b in zip(ins, outs)],
        "one_way_map": [[owm[2 * i].hex(), owm[2 * i + 1].hex()] for i in range(len(owm) // 2)],
        "hash_to_curve": {"dst": dst_ro, "vectors": kat_tuples(ed, "RFC_HASH_TO_CURVE_KAT", 2)},
        "encode_to_curve": {"dst": dst_nu, "vectors": kat_tuples(ed, "RFC_ENCODE_TO_CURVE_KAT", 2)},
        "hash_to_field_1": {"dst": dst_nu, "vectors": kat_tuples(fld, "RFC_HASH_TO_FIELD_KAT", 1)},
        "hash_to_field_2": {"dst": dst_ro, "vectors": kat_tuples(fld, "RFC_HASH_TO_FIELD_KAT_2", 2)},
    }
    for k in ("hash_to_curve", "encode_to_curve", "hash_to_field_1", "hash_to_field_2"):
        assert len(data[k]["vectors"]) == 5, (k, len(data[k]["vectors"]))
    with open(os.path.join(HERE, "h2c_vectors.json"), "w") as f:
        json.dump(data, f, indent=1)
        f.write("\n")
    print("h2c_vectors.json: %d sage pairs, %d one-way-map pairs, 4 x 5 RFC 9380 vectors" % (len(ins), len(owm) // 2))


if __name__ == "__main__":
    main()
