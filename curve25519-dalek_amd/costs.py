"""Field-operation counts of the hot path AS IMPLEMENTED, derived from the kernels' parameters -- the ONE table that
bench.py's `valu` objects and DESIGN.md section 4 both read (round 1 kept hand-typed constants in bench.py that drifted
from the code).

M = fe_mul (csrc/fe26.h: 100 v_mad_u64_u32 products + 1 for the 19*carry fold), S = fe_sq (55 + 1).  Every function
returns a dict {"M": .., "S": .., "what": ..} per UNIT of the workload (scalar, ladder, term, signature), and
`mac(cost)` turns it into 32x32->64 multiply-accumulates, the unit of the binding roof.
`reference_mac` holds SURVEY.md 8d's counts for the REFERENCE algorithm (5 x 51-bit schoolbook: M = 100, S = 60).

Formula sources (file:function):
  mixed addition                7 M      ge26.h:ge_madd_signed_p3
  first window by conversion    1 M      ge26.h:ge_from_aniels_signed
  complete addition             9 M      ge26.h:ge_add  (1 M to_cached + 4 M + 4 M)
  doubling to extended          4 S+4 M  ge26.h:ge_dbl + ge_p1p1_to_p3   (3 M when another doubling follows)
  inversion / pow_p58           254 S + 11 M / 251 S + 12 M              fe26.h:fe_invert, fe_pow_p58
  decompression                 255 S + 21 M                             ge26.h:ge_decompress (T = X*Y is dead code in the MSM prep)
  batched compression           5 M + inversion / 16                     finish.hip:k_compress_p32<16>
  affine Niels record           2 M (x*y, *2d)                           devio.h:pts_store
  sqrt_ratio_i                  254 S + 20 M                             ge26.h:fe_sqrt_ratio_i (pow_p58 + 8 M + 3 S around it)
  Ristretto Elligator map       256 S + 33 M                             h2c.h:ris_elligator
  Ristretto compression         255 S + 33 M                             ge26.h:ris_compress
  Elligator 2 + Edwards map     258 S + 36 M                             h2c.h:mont_elligator2 + ed_h2c_map
  Ristretto decompression       257 S + 27 M                             ge26.h:ris_decompress
  Jacobi quartic points (4)     258 S + 40 M                             lizard.h:ris_to_jacobi_quartic
  e_inv_positive                257 S + 23 M                             lizard.h:jacobi_e_inv_positive (8 per decode / inverse)
  Montgomery ladder step        5 M + 4 S + 0.1 M                        montgomery.h:mont_ladder_step (k_x25519, k_mont_mul, k_mont_mul_bits)
  to_edwards                    255 S + 26 M + inversion / 16            montgomery.hip:k_mont_to_edwards_prep + k_ratio_p32 + k_mont_to_edwards
  group law, elementwise        add / sub 9 M, neg 0, mul_by_cofactor 3 x (4 S + 3 M) + 1 M, eq 4 M   group.hip:k_group_elem, k_group_eq
  segmented sum                 (K + 7) / K additions per point (K = 8)  group.hip:k_seg_sum (serial fold of K, six scan steps, the carry-in)
"""
import math

MAC_PER_M = 100
MAC_PER_S = 55
INV = {"M": 11, "S": 254}          # fe_invert
CHUNK = 16                         # points per lane sharing one inversion (Montgomery's trick): compression, ladder output
PREP_CHUNK = 64                    # the same in the MSM's normaliser (msm.hip:k_prep_raw2<64>)

reference_mac = {"fixed_base": 47100, "x25519": 231000, "msm": 26500, "verify": 57000, "verify_bytes": 74400}


def mac(c):
    return MAC_PER_M * c["M"] + MAC_PER_S * c["S"]


def _add(*cs):
    return {"M": sum(c["M"] for c in cs), "S": sum(c["S"] for c in cs)}


def _scaled(c, f):
    return {"M": c["M"] * f, "S": c["S"] * f}


def compress_batch():
    """finish.hip:k_compress_p32<16>: prefix product 1 M, zi = inv*pre 1 M, inv*Z 1 M, X*zi, Y*zi 2 M, + 1/16 inversion."""
    return _add({"M": 5, "S": 0}, _scaled(INV, 1.0 / CHUNK))


def fixed_base_wide(C=16):
    """kernels.hip:k_mul_base_wide: ceil(256/C) windows, the first by conversion, no doublings; + batched compression."""
    nw = -(-256 // C)
    c = _add({"M": 1 + 7 * (nw - 1), "S": 0}, compress_batch())
    c["what"] = "1 M (first window) + %d madd x 7 M (radix-2^%d tables in HBM) + 5 M compress + 1/16 inversion" % (nw - 1, C)
    return c


def fixed_base_comb():
    """kernels.hip:k_mul_base_comb: 31 mixed additions (6 tables x 5 rows + the parity fix-up) + 4 doublings."""
    c = _add({"M": 31 * 7 + 4 * 4, "S": 4 * 4}, compress_batch())
    c["what"] = "31 madd x 7 M + 4 dbl x (4 S + 4 M) (LDS comb) + 5 M compress + 1/16 inversion"
    return c


def fixed_base_ct(W=5):
    """kernels.hip:k_mul_base_ctp<W> (round 5; rounds 2-4: k_mul_base<W, CT>): ceil(256/W) mixed additions; the table entry reaches the lane by a
    cross-lane fetch (LDS reads at lane-index addresses + ds_bpermute), which is not multiplier work and therefore not in this count."""
    nw = -(-256 // W)
    c = _add({"M": 7 * nw, "S": 0}, compress_batch())
    c["what"] = "%d madd x 7 M (radix-2^%d LDS tables, constant-time cross-lane fetch per lookup) + 5 M compress + 1/16 inversion" % (nw, W)
    return c


def x25519():
    """kernels.hip:k_x25519: 255 ladder steps of 5 M + 4 S + one 10-product small multiplication (0.1 M), then
    finish.hip:k_ratio_p32 (3 M + 1/16 inversion)."""
    c = _add({"M": 255 * 5.1, "S": 255 * 4}, {"M": 3, "S": 0}, _scaled(INV, 1.0 / CHUNK))
    c["what"] = "255 x (5 M + 4 S + 10-product a24 mul) + 3 M + 1/16 inversion"
    return c


def _reduce_per_bucket():
    """Bucket reduction sum_b (b+1) B_b, priced at its ALGORITHMIC minimum -- the running-sum method of
    pippenger.rs:146-151, two complete additions (9 M each) per bucket.  reduce.hip:k_reduce_a4 / k_reduce_b4 issue more
    (per 8 buckets: 13 serial additions, then 13 additions + 3 doublings of the wave-wide combine, i.e. 3.25 additions
    + 0.375 doublings per bucket) to cut the dependent chain from 2 x 32768 additions to 40; the surplus is overhead,
    not achieved work."""
    return {"M": 2 * 9, "S": 0}


def msm(n, nwin, half, raw_points=True, filled_windows=None):
    """One bucket-method pass over n terms with `nwin` windows of `half` buckets (c25519_msm_geometry).
    filled_windows: windows that hold a digit for a reduced (< 2^253) scalar: all but the overflow window."""
    fw = (nwin - 1) if filled_windows is None else filled_windows
    acc = {"M": 7 * fw, "S": 0}
    if raw_points:       # msm.hip:k_prep_raw2<64>: 1 M prefix, 2 M unwind, 2 M (x, y), 2 M record, + 1/64 inversion
        prep = _add({"M": 7, "S": 0}, _scaled(INV, 1.0 / PREP_CHUNK))
    else:                # kernels.hip:k_prep_compressed: decompression + record
        prep = {"M": 21 + 2, "S": 255}
    red = _scaled(_reduce_per_bucket(), float(nwin) * half / n)
    c = _add(acc, prep, red)
    c["what"] = "%d windows x 7 M bucket adds + %s + bucket reduction %.1f M-equivalents per term (%d x %d buckets)" % (
        fw, "7.2 M + 4 S normalise (1/64 inversion)" if raw_points else "decompress (255 S + 23 M)", (mac(red)) / 100.0, nwin, half)
    return c


def verify(n, nwin, half, keys_as_bytes=False, r_windows=8):
    """One verify_batch pass: R decompressed (255 S + 23 M incl. record), A from the cached point (Z = 1, as
    VerifyingKey::from_bytes leaves it: 1 M prefix product + 2 M record, msm.hip:k_prep_raw's affine path) or decompressed, R-terms in `r_windows` windows (|z| < 2^127), A-terms in nwin - 1; SHA-512 and the scalar
    arithmetic mod l are integer work outside this count."""
    a_prep = {"M": 23, "S": 255} if keys_as_bytes else {"M": 3, "S": 0}
    red = _scaled(_reduce_per_bucket(), float(nwin) * half / n)
    c = _add({"M": 23, "S": 255}, a_prep, {"M": 7 * (r_windows + nwin - 1), "S": 0}, red)
    c["what"] = "decompress R (255 S + 23 M) + %s + (%d + %d) windows x 7 M + bucket reduction; SHA-512 and scalar muls not counted" % (
        "decompress A (255 S + 23 M)" if keys_as_bytes else "A from VerifyingKey.point (Z = 1: 3 M)", r_windows, nwin - 1)
    return c


SQRT_RATIO = {"M": 20, "S": 254}
RIS_MAP = _add(SQRT_RATIO, {"M": 13, "S": 2})       # r = i r0^2 (1 S + 1 M), N_s, D (3 M), s' (1 M), N_t (2 M), s^2 (1 S), W (2 M), to extended (4 M)
RIS_COMPRESS = _add(SQRT_RATIO, {"M": 13, "S": 1})
ED_MAP = _add({"M": 12, "S": 251}, {"M": 24, "S": 7})  # pow_p58 of G.2.1 step 16 + the other 17 M + 7 S of G.2.1 + 7 M of the rational map
ADD = {"M": 9, "S": 0}


def ristretto_from_uniform(compressed=True):
    """h2c.hip:k_ristretto_from_uniform: two Elligator maps (three exponentiation chains with the compression), the sum."""
    c = _add(RIS_MAP, RIS_MAP, ADD, RIS_COMPRESS if compressed else {"M": 0, "S": 0})
    c["what"] = "2 Elligator maps (256 S + 33 M each) + 9 M sum" + (" + Ristretto compression (255 S + 33 M)" if compressed else " (RAW160 out)")
    return c


def edwards_hash_to_curve(ro=True):
    """h2c.hip:k_edwards_h2c<RO> + the batched compression; SHA-512 (4 compressions of expand_message_xmd for a short message, RO) is
    integer work outside this count."""
    c = _add(ED_MAP, ED_MAP if ro else {"M": 0, "S": 0}, ADD if ro else {"M": 0, "S": 0}, {"M": 10, "S": 12}, compress_batch())
    c["what"] = "%s Elligator 2 + Edwards map (258 S + 36 M)%s + x8 (12 S + 10 M) + 5 M compress + 1/16 inversion" % ("2 x" if ro else "1 x", " + 9 M sum" if ro else "")
    return c


RIS_DECOMPRESS = _add(SQRT_RATIO, {"M": 7, "S": 3})
JACOBI4 = _add(SQRT_RATIO, {"M": 20, "S": 4})       # 4 S of X^2 Y^2 Y^4 Z^2, 2 M into the invsqrt, 18 M of the s_i, t_i
E_INV = _add(SQRT_RATIO, {"M": 3, "S": 3})           # a, i (s^4 - a^2), x (3 M); a^2, s^2, s^4 (3 S)


def lizard_encode(compressed=True):
    """lizard.hip:k_lizard_encode: one Elligator map and the compression; SHA-256 (one compression) is integer work outside this count."""
    c = _add(RIS_MAP, RIS_COMPRESS if compressed else {"M": 0, "S": 0})
    c["what"] = "1 Elligator map (256 S + 33 M)" + (" + Ristretto compression (255 S + 33 M)" if compressed else " (RAW160 out)")
    return c


def lizard_decode(compressed=True):
    """lizard.hip:k_lizard_decode: (decompression,) the four Jacobi points, 8 e_inv_positive; 8 SHA-256 compressions are integer
    work outside this count.  Ten inverse square roots from compressed input, nine from RAW160."""
    c = _add(RIS_DECOMPRESS if compressed else {"M": 0, "S": 0}, JACOBI4, _scaled(E_INV, 8))
    c["what"] = ("decompression + " if compressed else "") + "4 Jacobi points (258 S + 40 M) + 8 x e_inv_positive (257 S + 23 M)"
    return c


def map_to_curve_inverse(compressed=True):
    """lizard.hip:k_map_to_curve_inverse: the field work of lizard_decode without the hashes"""
    c = lizard_decode(compressed)
    c["what"] = "as lizard_decode, 16 canonical encodings out instead of 8 hashes"
    return c


def montgomery_mul_bits(nbits=255):
    """montgomery.hip:k_mont_mul_bits (nbits = 255: k_mont_mul, the same count as x25519()): nbits ladder steps, then k_ratio_p32"""
    c = _add({"M": nbits * 5.1, "S": nbits * 4}, {"M": 3, "S": 0}, _scaled(INV, 1.0 / CHUNK))
    c["what"] = "%d x (5 M + 4 S + 10-product a24 mul) + 3 M + 1/16 inversion" % nbits
    return c


def montgomery_to_edwards():
    """montgomery.hip: y = (u - 1) / (u + 1) by the batched division of finish.hip:k_ratio_p32 (4 M + 1/16 inversion), then
    k_mont_to_edwards: the decompression (255 S + 22 M with T = X Y); the compression of the affine result is a canonical encoding, no
    field operation.  (The per-lane arm pays a whole inversion, 254 S + 11 M, and 1 M instead of the batched division.)"""
    c = _add({"M": 4, "S": 0}, _scaled(INV, 1.0 / CHUNK), {"M": 22, "S": 255})
    c["what"] = "batched division (4 M + 1/16 inversion) + decompression (255 S + 22 M)"
    return c


def group_elem(op="add", compressed=False):
    """group.hip:k_group_elem / k_group_eq per item: the operation (ge_add 9 M; ge_neg none; mul_by_cofactor two doublings to projective
    (4 S + 3 M each) and one to extended (4 S + 4 M); ge_eq 4 M), plus per compressed input one decompression (255 S + 22 M) and for a
    compressed output the batched compression (5 M + 1/16 inversion)"""
    ops = {"add": {"M": 9, "S": 0}, "neg": {"M": 0, "S": 0}, "mul_by_cofactor": {"M": 10, "S": 12}, "eq": {"M": 4, "S": 0}}
    inputs = 1 if op in ("neg", "mul_by_cofactor") else 2
    c = dict(ops[op])
    if compressed:
        c = _add(c, _scaled({"M": 22, "S": 255}, inputs))
        if op != "eq":
            c = _add(c, {"M": 5, "S": 0}, _scaled(INV, 1.0 / CHUNK))
    c["what"] = "%s%s" % (op, ", CompressedEdwardsY in and out" if compressed else ", RAW160")
    return c


def segmented_sum(k=8):
    """group.hip:k_seg_sum per point at level 0: one addition per point in the lane's serial fold, and per lane (k points) six scan steps
    and the carry-in addition; the piece levels add 2 / (64 k) of that again per level"""
    c = _scaled({"M": 9, "S": 0}, (k + 7.0) / k)
    c["what"] = "(K + 7) / K complete additions, K = %d" % k
    return c


def table():
    """Rows for DESIGN.md (python -m curve25519_dalek_amd.costs)."""
    rows = [("fixed base, radix 2^16 tables", fixed_base_wide(16)), ("fixed base, LDS comb", fixed_base_comb()),
            ("fixed base, constant-time scan W=5", fixed_base_ct(5)), ("X25519 ladder", x25519()),
            ("MSM 2^21 terms, raw points", msm(1 << 21, 17, 32768)), ("verify_batch 2^20, VerifyingKey", verify(1 << 20, 17, 32768)),
            ("verify_batch 2^20, keys as bytes", verify(1 << 20, 17, 32768, True)),
            ("Ristretto from_uniform_bytes", ristretto_from_uniform()), ("Edwards hash_to_curve (RO)", edwards_hash_to_curve()),
            ("Lizard encode", lizard_encode()), ("Lizard decode (compressed in)", lizard_decode()), ("map_to_curve_inverse", map_to_curve_inverse()),
            ("MontgomeryPoint mul / mul_bits_be 255", montgomery_mul_bits(255)), ("mul_bits_be 512", montgomery_mul_bits(512)),
            ("MontgomeryPoint::to_edwards", montgomery_to_edwards()),
            ("group add, RAW160", group_elem("add")), ("group add, compressed", group_elem("add", True)), ("group eq, RAW160", group_elem("eq")),
            ("segmented sum, per point", segmented_sum())]
    return [(name, round(c["M"], 1), round(c["S"], 1), int(round(mac(c))), c["what"]) for name, c in rows]


if __name__ == "__main__":
    for r in table():
        print("| %s | %s M + %s S | %d | %s |" % r)
