"""Host-side mirror of the reference's interface for the hot path (same names, argument meaning and
error behaviour), batched, on top of Engine.  Reference entry points mirrored:

  EdwardsPoint::mul_base                      curve25519-dalek/src/edwards.rs:918
  EdwardsPoint::vartime_multiscalar_mul       curve25519-dalek/src/traits.rs:249 / edwards.rs:1002
  RistrettoPoint::vartime_multiscalar_mul     curve25519-dalek/src/ristretto.rs:984
  EdwardsPoint / RistrettoPoint::vartime_multiscalar_mul, many independent sums in one call   (vartime_multiscalar_mul_many)
  CompressedEdwardsY::decompress / compress   edwards.rs:211 / :615
  x25519                                      x25519-dalek/src/x25519.rs:390
  verify_batch                                ed25519-dalek/src/batch.rs:146
  VerifyingKey::verify / verify_strict        ed25519-dalek/src/verifying.rs:565 / :359   (verify_each)
  SigningKey::sign                            ed25519-dalek/src/signing.rs:878-905        (sign_batch)
  VerifyingKey::verify_prehashed[_strict] / SigningKey::sign_prehashed   verifying.rs:284 / :424, signing.rs:312   (Ed25519ph: verify_each_prehashed, sign_batch_prehashed)
  EdwardsPoint::multiscalar_mul               curve25519-dalek/src/edwards.rs:966-1000
  VartimeEdwardsPrecomputation                curve25519-dalek/src/edwards.rs:1037-1076
  VartimeRistrettoPrecomputation              curve25519-dalek/src/ristretto.rs:1004
  Vartime{Edwards,Ristretto}Precomputation::vartime_multiscalar_mul, many rows of scalars over one precomputation in one call
                                              traits.rs:304-419   (vartime_multiscalar_mul_many)
  Vartime{Edwards,Ristretto}Precomputation::vartime_mixed_multiscalar_mul, many rows of static scalars plus each row's own dynamic terms in one call
                                              traits.rs:304-419, precomputed_straus.rs:29-127   (vartime_mixed_multiscalar_mul_many)
  the random-linear-combination fold of many such equations into ONE multiscalar mul, as ed25519-dalek/src/batch.rs:207-233 folds signatures
                                              (vartime_mixed_multiscalar_mul_folded; without a precomputation vartime_multiscalar_mul_folded)
  RistrettoPoint::double_and_compress_batch   curve25519-dalek/src/ristretto.rs:564
  Scalar::invert_batch                        curve25519-dalek/src/scalar.rs:802
  EdwardsBasepointTable::create / mul_base    curve25519-dalek/src/edwards.rs:1131-1141 / :1192-1209   (any basepoint)
  RistrettoBasepointTable::create             curve25519-dalek/src/ristretto.rs:1080-1110
  EdwardsPoint::mul_base_clamped / mul_clamped   curve25519-dalek/src/edwards.rs:948 / :932
  SharedSecret::was_contributory              x25519-dalek/src/x25519.rs:335
  RistrettoPoint::from_uniform_bytes / map_to_curve / hash_from_bytes::<Sha512>   ristretto.rs:774 / elligator.rs:62 / ristretto.rs:736
  EdwardsPoint::hash_to_curve / encode_to_curve::<Sha512>   curve25519-dalek/src/edwards.rs:710-750 (RFC 9380)
  RistrettoPoint::lizard_encode / lizard_decode::<Sha256>, map_to_curve_inverse, map_to_curve_restricted
                                              curve25519-dalek/src/lizard/lizard_ristretto.rs:25 / :46 / :232 / :215 (feature `lizard`)
  MontgomeryPoint::mul (Mul<&Scalar>) / mul_bits_be / mul_base / to_edwards / mul_clamped / mul_base_clamped
                                              curve25519-dalek/src/montgomery.rs:484 / :183 / :144 / :239 / :150 / :166
  EdwardsPoint::is_small_order / is_torsion_free   curve25519-dalek/src/edwards.rs:1405 / :1435;  VerifyingKey::is_weak  ed25519-dalek/src/verifying.rs:192
  EdwardsPoint / RistrettoPoint Add, Sub, Neg, ConstantTimeEq, is_identity, Sum (add, sub, neg, ct_eq, is_identity, sum, sum_segments),
  EdwardsPoint::mul_by_cofactor, Mul<&Scalar>    edwards.rs:501 / :808-875 / :1365 / :890, ristretto.rs:815 / :852-907 / :910
  RistrettoPoint::vartime_double_scalar_mul_basepoint   curve25519-dalek/src/ristretto.rs:1054

Values cross this layer as the reference's wire types: Scalar = 32 canonical LE bytes,
CompressedEdwardsY / CompressedRistretto / MontgomeryPoint = 32 bytes.
"""
import numpy as np

from . import engine as _e


class DomainSeparatorError(ValueError):
    """hash_to_curve / encode_to_curve with an empty domain separator or one longer than 255 bytes (a panic in the reference,
    field.rs:457-462)"""


def _joined(x):
    """bytes, or a sequence of byte pieces concatenated -- the reference's `&[&[u8]]`"""
    if isinstance(x, (bytes, bytearray, memoryview)):
        return bytes(x)
    return b"".join(bytes(p) for p in x)


class SignatureError(Exception):
    """ed25519-dalek/src/errors.rs:21-42 InternalError, by name."""

    def __init__(self, kind):
        super().__init__(kind)
        self.kind = kind


_ENGINE = None


def default_engine():
    global _ENGINE
    if _ENGINE is None:
        _ENGINE = _e.Engine()
    return _ENGINE


def _cat(items, width):
    if len(items) == 0:
        return np.zeros((0, width), dtype=np.uint8)
    return np.frombuffer(b"".join(bytes(x) for x in items), dtype=np.uint8).reshape(-1, width)


def _edwards_h2c(messages, domain_sep, mode, engine):
    dst = _joined(domain_sep)
    if not 0 < len(dst) <= 255:
        raise DomainSeparatorError("domain separator must have 1 .. 255 bytes, got %d" % len(dst))
    eng = engine or default_engine()
    out = eng.edwards_hash_to_curve_batch([_joined(m) for m in messages], dst, mode, _e.FMT_EDWARDS_Y)
    return [out[i].tobytes() for i in range(out.shape[0])]


class EdwardsPoint:
    @staticmethod
    def mul_base(scalars, engine=None):
        """[s_i * B] as CompressedEdwardsY bytes (edwards.rs:918 followed by compress :615)."""
        eng = engine or default_engine()
        out = eng.mul_base_batch(_cat(scalars, 32), _e.FMT_EDWARDS_Y)
        return [out[i].tobytes() for i in range(out.shape[0])]

    @staticmethod
    def vartime_multiscalar_mul(scalars, points, engine=None):
        """sum s_i P_i with P_i given as CompressedEdwardsY; returns CompressedEdwardsY bytes, or None
        if a point does not decompress (optional_multiscalar_mul, edwards.rs:1002-1031).  Unequal
        lengths raise, like the reference's assert_eq! (edwards.rs:1017-1019)."""
        if len(scalars) != len(points):
            raise AssertionError("vartime_multiscalar_mul: scalars and points must have equal length")
        eng = engine or default_engine()
        st, out = eng.msm_vartime(_cat(scalars, 32), _cat(points, 32), _e.FMT_EDWARDS_Y, _e.FMT_EDWARDS_Y)
        return None if st == _e.NONE else out

    @staticmethod
    def vartime_multiscalar_mul_many(scalar_lists, point_lists, engine=None):
        """[vartime_multiscalar_mul(scalar_lists[k], point_lists[k])] for every k in one call: CompressedEdwardsY bytes, or None where a
        point of that sum does not decompress.  Unequal lengths inside a pair raise, as in the single form.  Sums of up to
        engine.MSM_SEGMENT_BUCKET_MAX terms all run inside the one call: one GPU lane or one wave each up to engine.MSM_SEGMENT_WAVE_MAX terms
        (Bulletproofs-size equations included), the bucket method side by side beyond (aggregated range proofs); a still longer one costs a
        single-MSM call of its own (Engine.msm_vartime_segments_routes tells which)."""
        return _msm_many(scalar_lists, point_lists, _e.FMT_EDWARDS_Y, engine)

    @staticmethod
    def vartime_multiscalar_mul_folded(scalar_lists, point_lists, weights, engine=None):
        """sum_k weights[k] * vartime_multiscalar_mul(scalar_lists[k], point_lists[k]) as ONE multiscalar mul (every scalar times its sum's
        weight mod l, the fold of ed25519-dalek/src/batch.rs:207-233): CompressedEdwardsY bytes, or None if a point does not decompress.
        weights: one 16-byte (128-bit, as batch.rs draws them) or 32-byte little-endian integer per sum.  The equations sum_i s_i P_i = 0 all
        hold iff (up to the weights' randomness) the result is the identity encoding.  Exact for torsion-free points; a point with torsion
        changes the result by a small-order point, as in verify_batch."""
        return _msm_folded(scalar_lists, point_lists, weights, _e.FMT_EDWARDS_Y, engine)

    @staticmethod
    def vartime_double_scalar_mul_basepoint(a, A, b, engine=None):
        """[a_i * A_i + b_i * B] (edwards.rs:1099-1106 over vartime_double_base.rs:23-72), batched: A_i as
        160-byte raw EdwardsPoints, results as CompressedEdwardsY bytes."""
        if not (len(a) == len(A) == len(b)):
            raise AssertionError("vartime_double_scalar_mul_basepoint: a, A, b must have equal length")
        eng = engine or default_engine()
        out, _ = eng.double_base_batch(_cat(a, 32), _cat(A, 160), _cat(b, 32), _e.FMT_RAW160, _e.FMT_EDWARDS_Y)
        return [out[i].tobytes() for i in range(out.shape[0])]


    @staticmethod
    def mul_base_clamped(raw_bytes, engine=None):
        """[clamp_integer(b_i) * B] as CompressedEdwardsY bytes (edwards.rs:948-956; the clamped integer is not reduced mod l)."""
        eng = engine or default_engine()
        out = eng.mul_base_clamped_batch(_cat(raw_bytes, 32), _e.FMT_EDWARDS_Y)
        return [out[i].tobytes() for i in range(out.shape[0])]

    @staticmethod
    def mul_clamped(points, raw_bytes, engine=None):
        """[clamp_integer(b_i) * P_i] (edwards.rs:932-946): P_i as CompressedEdwardsY, results likewise; None where P_i does not decode."""
        if len(points) != len(raw_bytes):
            raise AssertionError("mul_clamped: points and scalars must have equal length")
        eng = engine or default_engine()
        out, ok = eng.mul_clamped_batch(_cat(raw_bytes, 32), _cat(points, 32), _e.FMT_EDWARDS_Y, _e.FMT_EDWARDS_Y)
        return [out[i].tobytes() if ok[i] else None for i in range(out.shape[0])]

    # the group law (edwards.rs:501-520, :808-875, :1365, :1484) and EdwardsPoint * Scalar (edwards.rs:890-911): CompressedEdwardsY bytes
    # in and out (ZIP-215 decoding), None where an input does not decode
    @staticmethod
    def add(ps, qs, engine=None):
        return _group_add(ps, qs, _e.POINT_ADD, _e.FMT_EDWARDS_Y, "add", engine)

    @staticmethod
    def sub(ps, qs, engine=None):
        return _group_add(ps, qs, _e.POINT_SUB, _e.FMT_EDWARDS_Y, "sub", engine)

    @staticmethod
    def neg(ps, engine=None):
        return _group_map(ps, _e.POINT_NEG, _e.FMT_EDWARDS_Y, engine)

    @staticmethod
    def mul_by_cofactor(ps, engine=None):
        return _group_map(ps, _e.POINT_MUL_BY_COFACTOR, _e.FMT_EDWARDS_Y, engine)

    @staticmethod
    def ct_eq(ps, qs, engine=None):
        """[P_i == Q_i] (ConstantTimeEq, edwards.rs:501-512: projective equality of the decoded points); None where one does not decode"""
        return _group_eq(ps, qs, _e.FMT_EDWARDS_Y, "ct_eq", engine)

    @staticmethod
    def is_identity(ps, engine=None):
        return _group_eq(ps, None, _e.FMT_EDWARDS_Y, "is_identity", engine)

    @staticmethod
    def sum(ps, engine=None):
        """sum of one list (impl Sum, edwards.rs:837-851); the identity for an empty list, None if a point does not decode"""
        return _group_sum_segments(ps, [len(ps)], _e.FMT_EDWARDS_Y, engine)[0]

    @staticmethod
    def sum_segments(ps, lengths, engine=None):
        """[sum of the next lengths[s] points of ps] for every s: many independent sums in one call"""
        return _group_sum_segments(ps, lengths, _e.FMT_EDWARDS_Y, engine)

    @staticmethod
    def mul(points, scalars, engine=None):
        """[P_i * s_i] (edwards.rs:890-911), constant-time unless the engine was made with FLAG_VARTIME_TABLES"""
        return _group_mul(points, scalars, _e.FMT_EDWARDS_Y, engine)

    @staticmethod
    def hash_to_curve(messages, domain_sep, engine=None):
        """[EdwardsPoint::hash_to_curve::<Sha512>(msg_i, domain_sep)] as CompressedEdwardsY bytes (edwards.rs:736-750, RFC 9380
        edwards25519_XMD:SHA-512_ELL2_RO_).  Each message and the DST: bytes, or a list of pieces concatenated (the reference's
        &[&[u8]]).  An empty DST or one longer than 255 bytes raises DomainSeparatorError (the reference panics)."""
        return _edwards_h2c(messages, domain_sep, _e.H2C_RO, engine)

    @staticmethod
    def encode_to_curve(messages, domain_sep, engine=None):
        """[EdwardsPoint::encode_to_curve::<Sha512>(msg_i, domain_sep)] (edwards.rs:710-734, ..._ELL2_NU_), arguments as hash_to_curve"""
        return _edwards_h2c(messages, domain_sep, _e.H2C_NU, engine)


def _order_flags(points, which, engine):
    eng = engine or default_engine()
    return eng.point_order_checks(_cat(points, 32), _e.FMT_EDWARDS_Y, which)


def is_small_order(points, engine=None):
    """[CompressedEdwardsY] -> [EdwardsPoint::is_small_order(), or None where the encoding does not decode] (edwards.rs:1405)"""
    fl = _order_flags(points, _e.POINT_SMALL_ORDER, engine)
    return [bool(f & _e.POINT_SMALL_ORDER) if f & _e.POINT_DECODES else None for f in fl]


def is_torsion_free(points, engine=None):
    """[CompressedEdwardsY] -> [EdwardsPoint::is_torsion_free(), or None] (edwards.rs:1435)"""
    fl = _order_flags(points, _e.POINT_TORSION_FREE, engine)
    return [bool(f & _e.POINT_TORSION_FREE) if f & _e.POINT_DECODES else None for f in fl]


class EdwardsBasepointTable:
    """edwards.rs:1125-1209 for ANY basepoint: `create(&P)` builds the window table once, `mul_base(&s)` = `&s * &table`
    multiplies secret scalars by P with constant-time table lookups (window.rs:54-76 semantics) whatever the engine's flags."""

    _fmt = _e.FMT_EDWARDS_Y

    def __init__(self, basepoint, engine=None):
        self.eng = engine or default_engine()
        self.point = bytes(basepoint)
        self.h = self.eng.basetable_create(self.point, self._fmt)

    @classmethod
    def create(cls, basepoint, engine=None):
        return cls(basepoint, engine)

    def basepoint(self):
        return self.point

    def mul_base(self, scalars):
        out = self.eng.mul_table_batch(self.h, _cat(scalars, 32), self._fmt)
        return [out[i].tobytes() for i in range(out.shape[0])]

    def close(self):
        if self.h:
            self.eng.basetable_destroy(self.h)
            self.h = None


class RistrettoBasepointTable(EdwardsBasepointTable):
    """ristretto.rs:1080-1110: the same table over a CompressedRistretto basepoint, results as CompressedRistretto."""
    _fmt = _e.FMT_RISTRETTO


class RistrettoPoint:
    @staticmethod
    def vartime_multiscalar_mul(scalars, points, engine=None):
        """ristretto.rs:984: points and result as CompressedRistretto bytes."""
        if len(scalars) != len(points):
            raise AssertionError("vartime_multiscalar_mul: scalars and points must have equal length")
        eng = engine or default_engine()
        st, out = eng.msm_vartime(_cat(scalars, 32), _cat(points, 32), _e.FMT_RISTRETTO, _e.FMT_RISTRETTO)
        return None if st == _e.NONE else out

    @staticmethod
    def vartime_multiscalar_mul_many(scalar_lists, point_lists, engine=None):
        """[vartime_multiscalar_mul(scalar_lists[k], point_lists[k])] for every k in one call: CompressedRistretto bytes, or None; routed by
        length as EdwardsPoint.vartime_multiscalar_mul_many"""
        return _msm_many(scalar_lists, point_lists, _e.FMT_RISTRETTO, engine)

    @staticmethod
    def vartime_multiscalar_mul_folded(scalar_lists, point_lists, weights, engine=None):
        """EdwardsPoint.vartime_multiscalar_mul_folded over CompressedRistretto points (exact: the Ristretto group has prime order l)"""
        return _msm_folded(scalar_lists, point_lists, weights, _e.FMT_RISTRETTO, engine)

    @staticmethod
    def from_uniform_bytes(inputs, engine=None):
        """[RistrettoPoint::from_uniform_bytes(b_i).compress()] for 64-byte inputs (ristretto.rs:774)"""
        _check_width(inputs, 64, "from_uniform_bytes")
        eng = engine or default_engine()
        out = eng.ristretto_from_uniform_bytes_batch(_cat(inputs, 64), _e.FMT_RISTRETTO)
        return [out[i].tobytes() for i in range(out.shape[0])]

    @staticmethod
    def map_to_curve(inputs, engine=None):
        """[RistrettoPoint::map_to_curve(b_i).compress()] for 32-byte inputs (ristretto/elligator.rs:62-68: bit 255 ignored)"""
        _check_width(inputs, 32, "map_to_curve")
        eng = engine or default_engine()
        out = eng.ristretto_map_to_curve_batch(_cat(inputs, 32), _e.FMT_RISTRETTO)
        return [out[i].tobytes() for i in range(out.shape[0])]

    @staticmethod
    def hash_from_bytes(messages, engine=None):
        """[RistrettoPoint::hash_from_bytes::<Sha512>(m_i).compress()] (ristretto.rs:736-761); a message may be a list of pieces"""
        eng = engine or default_engine()
        out = eng.ristretto_hash_from_bytes_batch([_joined(m) for m in messages], _e.FMT_RISTRETTO)
        return [out[i].tobytes() for i in range(out.shape[0])]

    @staticmethod
    def lizard_encode(datas, engine=None):
        """[RistrettoPoint::lizard_encode::<Sha256>(d_i).compress()] for 16-byte payloads (lizard_ristretto.rs:25-42)"""
        _check_width(datas, 16, "lizard_encode")
        eng = engine or default_engine()
        out = eng.ristretto_lizard_encode_batch(_cat(datas, 16), _e.FMT_RISTRETTO)
        return [out[i].tobytes() for i in range(out.shape[0])]

    @staticmethod
    def lizard_decode(encodings, engine=None):
        """[CompressedRistretto(b_i).decompress().and_then(|p| p.lizard_decode::<Sha256>())]: 16 bytes, or None for an invalid
        encoding or a point without a unique Lizard preimage (lizard_ristretto.rs:46-75)"""
        _check_width(encodings, 32, "lizard_decode")
        eng = engine or default_engine()
        out, st = eng.ristretto_lizard_decode_batch(_cat(encodings, 32), _e.FMT_RISTRETTO)
        return [out[i].tobytes() if st[i] == _e.LIZARD_OK else None for i in range(out.shape[0])]

    @staticmethod
    def map_to_curve_inverse(encodings, engine=None):
        """[decompress(b_i).map_to_curve_inverse()] (lizard_ristretto.rs:232-238): per point a list of 16 `bytes | None` in the
        reference's slot order for the decompressed representative (slots 0..7 even, 8..15 their negations); None in place of
        the list for an invalid encoding (decompress() returned None)."""
        _check_width(encodings, 32, "map_to_curve_inverse")
        eng = engine or default_engine()
        out, mask, ok = eng.ristretto_map_to_curve_inverse_batch(_cat(encodings, 32), _e.FMT_RISTRETTO)
        return [[out[i, j].tobytes() if mask[i] >> j & 1 else None for j in range(16)] if ok[i] else None for i in range(out.shape[0])]

    @staticmethod
    def map_to_curve_restricted(inputs, engine=None):
        """[RistrettoPoint::map_to_curve_restricted(b_i).compress()] (lizard_ristretto.rs:215-224): ValueError where the reference
        panics, i.e. when the bottom bit of b[0] or one of the top two bits of b[31] is set"""
        _check_width(inputs, 32, "map_to_curve_restricted")
        for i, b in enumerate(inputs):
            if b[0] & 0x01 or b[31] & 0xC0:
                raise ValueError("map_to_curve_restricted: input %d has the bottom bit or one of the top two bits set" % i)
        return RistrettoPoint.map_to_curve(inputs, engine=engine)

    # the group law and scalar multiplication (ristretto.rs:809-935, :1054, :1197): CompressedRistretto bytes in and out, None where an
    # input does not decode
    @staticmethod
    def add(ps, qs, engine=None):
        return _group_add(ps, qs, _e.POINT_ADD, _e.FMT_RISTRETTO, "add", engine)

    @staticmethod
    def sub(ps, qs, engine=None):
        return _group_add(ps, qs, _e.POINT_SUB, _e.FMT_RISTRETTO, "sub", engine)

    @staticmethod
    def neg(ps, engine=None):
        return _group_map(ps, _e.POINT_NEG, _e.FMT_RISTRETTO, engine)

    @staticmethod
    def ct_eq(ps, qs, engine=None):
        """[P_i == Q_i] (ConstantTimeEq, ristretto.rs:815-830: equality of the group elements, not of the bytes); None where one does not decode"""
        return _group_eq(ps, qs, _e.FMT_RISTRETTO, "ct_eq", engine)

    @staticmethod
    def is_identity(ps, engine=None):
        return _group_eq(ps, None, _e.FMT_RISTRETTO, "is_identity", engine)

    @staticmethod
    def sum(ps, engine=None):
        """sum of one list (impl Sum, ristretto.rs:882-895); the identity for an empty list, None if a point does not decode"""
        return _group_sum_segments(ps, [len(ps)], _e.FMT_RISTRETTO, engine)[0]

    @staticmethod
    def sum_segments(ps, lengths, engine=None):
        """[sum of the next lengths[s] points of ps] for every s: many independent sums in one call"""
        return _group_sum_segments(ps, lengths, _e.FMT_RISTRETTO, engine)

    @staticmethod
    def mul(points, scalars, engine=None):
        """[P_i * s_i] (RistrettoPoint * Scalar, ristretto.rs:910-935), constant-time unless the engine was made with FLAG_VARTIME_TABLES"""
        return _group_mul(points, scalars, _e.FMT_RISTRETTO, engine)

    @staticmethod
    def vartime_double_scalar_mul_basepoint(a, A, b, engine=None):
        """[a_i * A_i + b_i * B] (ristretto.rs:1054): A_i as CompressedRistretto; None where A_i does not decode"""
        if not (len(a) == len(A) == len(b)):
            raise AssertionError("vartime_double_scalar_mul_basepoint: a, A, b must have equal length")
        eng = engine or default_engine()
        out, ok = eng.double_base_batch(_cat(a, 32), _cat(A, 32), _cat(b, 32), _e.FMT_RISTRETTO, _e.FMT_RISTRETTO)
        return [out[i].tobytes() if ok[i] else None for i in range(out.shape[0])]


def _msm_many(scalar_lists, point_lists, fmt, engine):
    if len(scalar_lists) != len(point_lists) or any(len(s) != len(p) for s, p in zip(scalar_lists, point_lists)):
        raise AssertionError("vartime_multiscalar_mul: scalars and points must have equal length")
    off = np.zeros(len(scalar_lists) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in scalar_lists], dtype=np.uint64)
    eng = engine or default_engine()
    _, out, ok = eng.msm_vartime_segments(_cat([x for s in scalar_lists for x in s], 32), _cat([x for p in point_lists for x in p], 32), off, fmt, fmt)
    return [out[i].tobytes() if ok[i] else None for i in range(out.shape[0])]


def _weights(weights, m):
    """m weights of one width, 16 or 32 bytes -> (m, width) uint8"""
    weights = [bytes(x) for x in weights]
    if len(weights) != m:
        raise AssertionError("folded multiscalar mul: one weight per row")
    width = len(weights[0]) if weights else 16
    if width not in (16, 32) or any(len(x) != width for x in weights):
        raise AssertionError("folded multiscalar mul: weights must all have 16 or all have 32 bytes")
    return _cat(weights, width)


def _msm_folded(scalar_lists, point_lists, weights, fmt, engine):
    if len(scalar_lists) != len(point_lists) or any(len(s) != len(p) for s, p in zip(scalar_lists, point_lists)):
        raise AssertionError("vartime_multiscalar_mul: scalars and points must have equal length")
    m = len(scalar_lists)
    off = np.zeros(m + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in scalar_lists], dtype=np.uint64)
    eng = engine or default_engine()
    st, out = eng.precomp_msm_vartime_mixed_rows_fold(None, np.zeros((m, 0, 32), np.uint8), _cat([x for s in scalar_lists for x in s], 32),
                                                      _cat([x for p in point_lists for x in p], 32), off, _weights(weights, m), fmt, fmt)
    return None if st == _e.NONE else out


def _group_add(ps, qs, op, fmt, what, engine):
    if len(ps) != len(qs):
        raise AssertionError("%s: both lists must have equal length" % what)
    eng = engine or default_engine()
    _, out, ok = eng.point_add_batch(_cat(ps, 32), _cat(qs, 32), op, fmt, fmt)
    return [out[i].tobytes() if ok[i] else None for i in range(out.shape[0])]


def _group_map(ps, op, fmt, engine):
    eng = engine or default_engine()
    _, out, ok = eng.point_map_batch(_cat(ps, 32), op, fmt, fmt)
    return [out[i].tobytes() if ok[i] else None for i in range(out.shape[0])]


def _group_eq(ps, qs, fmt, what, engine):
    if qs is not None and len(ps) != len(qs):
        raise AssertionError("%s: both lists must have equal length" % what)
    eng = engine or default_engine()
    _, eq, ok = eng.point_eq_batch(_cat(ps, 32), _cat(qs, 32) if qs is not None else None, fmt, fmt)
    return [bool(eq[i]) if ok[i] else None for i in range(eq.shape[0])]


def _group_sum_segments(ps, lengths, fmt, engine):
    lengths = [int(x) for x in lengths]
    if any(x < 0 for x in lengths) or sum(lengths) != len(ps):
        raise AssertionError("sum_segments: the lengths must be non-negative and add up to the number of points")
    off = np.zeros(len(lengths) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lengths, dtype=np.uint64)
    eng = engine or default_engine()
    _, out, ok = eng.point_sum_segments(_cat(ps, 32), off, fmt, fmt)
    return [out[i].tobytes() if ok[i] else None for i in range(out.shape[0])]


def _group_mul(points, scalars, fmt, engine):
    if len(points) != len(scalars):
        raise AssertionError("mul: points and scalars must have equal length")
    eng = engine or default_engine()
    out, ok = eng.mul_batch(_cat(scalars, 32), _cat(points, 32), fmt, fmt)
    return [out[i].tobytes() if ok[i] else None for i in range(out.shape[0])]


class MontgomeryPoint:
    """montgomery.rs, batched.  Points cross as MontgomeryPoint bytes (32-byte u-coordinates, decoded as FieldElement::from_bytes),
    scalars as 32 bytes taken as given (the reference's Scalar holds a reduced value; the ladder skips bit 255 either way)."""

    @staticmethod
    def mul(points, scalars, engine=None):
        """[&P_i * &s_i] (Mul<&Scalar>, montgomery.rs:484-492): the ladder over bits 254..0 of s_i, unclamped"""
        _check_width(points, 32, "MontgomeryPoint.mul"); _check_width(scalars, 32, "MontgomeryPoint.mul")
        if len(points) != len(scalars):
            raise ValueError("MontgomeryPoint.mul: points and scalars must have equal length")
        eng = engine or default_engine()
        out = eng.montgomery_mul_batch(_cat(scalars, 32), _cat(points, 32))
        return [out[i].tobytes() for i in range(out.shape[0])]

    @staticmethod
    def mul_bits_be(points, bits, engine=None):
        """[P_i.mul_bits_be(bits_i)] (montgomery.rs:183-211): bits_i is a sequence of bools, most significant first, the same
        length (at most 512) for every item"""
        nbits = len(bits[0]) if len(bits) else 0
        if any(len(b) != nbits for b in bits):
            raise ValueError("MontgomeryPoint.mul_bits_be: every bit string must have the same length")
        if nbits > _e.MONTGOMERY_MAX_BITS:
            raise ValueError("MontgomeryPoint.mul_bits_be: at most %d bits" % _e.MONTGOMERY_MAX_BITS)
        _check_width(points, 32, "MontgomeryPoint.mul_bits_be")
        if len(points) != len(bits):
            raise ValueError("MontgomeryPoint.mul_bits_be: points and bit strings must have equal length")
        packed = np.packbits(np.asarray(bits, dtype=bool).reshape(len(bits), nbits), axis=1) if nbits else np.empty((len(bits), 0), np.uint8)
        eng = engine or default_engine()
        out = eng.montgomery_mul_bits_be_batch(packed, nbits, _cat(points, 32))
        return [out[i].tobytes() for i in range(out.shape[0])]

    @staticmethod
    def mul_base(scalars, engine=None):
        """[MontgomeryPoint::mul_base(&s_i)] = EdwardsPoint::mul_base(s_i).to_montgomery() (montgomery.rs:144-146), unclamped"""
        _check_width(scalars, 32, "MontgomeryPoint.mul_base")
        eng = engine or default_engine()
        out = eng.montgomery_mul_base_batch(_cat(scalars, 32))
        return [out[i].tobytes() for i in range(out.shape[0])]

    @staticmethod
    def mul_clamped(points, raw_bytes, engine=None):
        """[P_i.mul_clamped(bytes_i)] (montgomery.rs:150-162): the X25519 ladder"""
        if len(points) != len(raw_bytes):
            raise ValueError("MontgomeryPoint.mul_clamped: points and scalars must have equal length")
        return x25519(raw_bytes, points, engine=engine)

    @staticmethod
    def mul_base_clamped(raw_bytes, engine=None):
        """[MontgomeryPoint::mul_base_clamped(bytes_i)] (montgomery.rs:166-174): the X25519 public-key path"""
        return x25519_public_keys(raw_bytes, engine=engine)

    @staticmethod
    def to_edwards(points, signs, engine=None):
        """[P_i.to_edwards(sign_i).map(|e| e.compress())] (montgomery.rs:239-268): 32 bytes, or None where the reference returns None
        (u = -1, or u on the twist); sign_i is a u8, of which only bit 0 counts"""
        _check_width(points, 32, "MontgomeryPoint.to_edwards")
        if len(points) != len(signs):
            raise ValueError("MontgomeryPoint.to_edwards: points and signs must have equal length")
        eng = engine or default_engine()
        out, st = eng.montgomery_to_edwards_batch(_cat(points, 32), np.asarray(signs, dtype=np.uint8), _e.FMT_EDWARDS_Y)
        return [out[i].tobytes() if st[i] else None for i in range(out.shape[0])]


def _check_width(items, width, what):
    for i, it in enumerate(items):
        if len(it) != width:
            raise ValueError("%s: input %d has %d bytes, expected %d" % (what, i, len(it), width))


class CompressedEdwardsY:
    @staticmethod
    def decompress(encodings, engine=None):
        """-> list of 160-byte raw EdwardsPoints or None (edwards.rs:211-258)."""
        eng = engine or default_engine()
        _, pts, ok = eng.decompress_batch(_cat(encodings, 32), _e.FMT_EDWARDS_Y)
        return [pts[i].tobytes() if ok[i] else None for i in range(len(encodings))]


def x25519(ks, us, engine=None):
    """x25519-dalek/src/x25519.rs:390, batched."""
    eng = engine or default_engine()
    out = eng.x25519_batch(_cat(ks, 32), _cat(us, 32))
    return [out[i].tobytes() for i in range(out.shape[0])]


class SharedSecret:
    """x25519-dalek/src/x25519.rs:301-345: the 32 bytes of a Diffie-Hellman result and was_contributory() (:335)."""
    __slots__ = ("bytes", "contributory")

    def __init__(self, b, contributory):
        self.bytes, self.contributory = bytes(b), bool(contributory)

    def as_bytes(self):
        return self.bytes

    def was_contributory(self):
        return self.contributory


def diffie_hellman(secrets, their_publics, engine=None):
    """StaticSecret::diffie_hellman (x25519.rs:219-222), batched -> [SharedSecret]"""
    eng = engine or default_engine()
    out, fl = eng.x25519_contributory_batch(_cat(secrets, 32), _cat(their_publics, 32))
    return [SharedSecret(out[i].tobytes(), fl[i]) for i in range(out.shape[0])]


class VerifyingKey:
    """ed25519-dalek/src/verifying.rs:64-71: the 32 key bytes together with the decompressed point, so that
    verify_batch does not decompress A_i again (batch.rs:236)."""
    __slots__ = ("compressed", "point")
    _from_bytes_token = object()

    def __init__(self, compressed, point, _token=None):
        # the type invariant of the reference (point == decompress(compressed)) is what verify_batch relies on when it
        # hashes the bytes and multiplies the point: only from_bytes, which computes the point itself, may build one
        if _token is not VerifyingKey._from_bytes_token:
            raise TypeError("VerifyingKey objects are built by VerifyingKey.from_bytes (verifying.rs:167-175)")
        self.compressed, self.point = bytes(compressed), bytes(point)

    @staticmethod
    def is_weak(keys, engine=None):
        """VerifyingKey::is_weak (verifying.rs:192-194) for a list of VerifyingKey: the point has small order"""
        eng = engine or default_engine()
        fl = eng.point_order_checks(_cat([k.point for k in keys], 160), _e.FMT_RAW160, _e.POINT_SMALL_ORDER)
        return [bool(f & _e.POINT_SMALL_ORDER) for f in fl]

    @staticmethod
    def from_bytes(keys, engine=None):
        """VerifyingKey::from_bytes (verifying.rs:167-175), batched: a list of VerifyingKey; raises
        SignatureError("PointDecompression") if any key does not decode."""
        eng = engine or default_engine()
        _, pts, ok = eng.decompress_batch(_cat(keys, 32), _e.FMT_EDWARDS_Y)
        if len(keys) and not ok.all():
            raise SignatureError("PointDecompression")
        return [VerifyingKey(keys[i], pts[i].tobytes(), VerifyingKey._from_bytes_token) for i in range(len(keys))]

    def as_bytes(self):
        return self.compressed

    def __bytes__(self):
        return self.compressed


def verify_batch(messages, signatures, verifying_keys, engine=None, z_mode=_e.Z_TRANSCRIPT):
    """ed25519-dalek/src/batch.rs:146: returns None on success, raises SignatureError otherwise
    (ArrayLength / ScalarFormat / Verify in the reference's precedence; PointDecompression for a key
    that would have failed VerifyingKey::from_bytes, verifying.rs:167).  verifying_keys: 32-byte strings, or
    VerifyingKey objects (then their cached points are used, as in the reference)."""
    eng = engine or default_engine()
    keys = list(verifying_keys)
    pk_points = None
    if keys and all(isinstance(k, VerifyingKey) for k in keys):
        pk_points = _cat([k.point for k in keys], 160)
    st = eng.verify_batch(list(messages), list(signatures), [bytes(k) for k in keys], z_mode, pk_points=pk_points)
    if st == _e.OK:
        return None
    raise SignatureError({_e.ARRAY_LENGTH: "ArrayLength", _e.SCALAR_FORMAT: "ScalarFormat", _e.VERIFY: "Verify",
                          _e.NONE: "PointDecompression"}[st])


def verify_batch_segments(batches, engine=None, z_mode=_e.Z_TRANSCRIPT):
    """verify_batch (batch.rs:146) over MANY independent batches in one GPU call.  batches: a list of (messages, signatures, verifying_keys)
    triples -> one entry per batch: None for Ok(()) or the SignatureError verify_batch would raise for that batch alone.  A triple of
    unequal lengths gives ArrayLength without touching the others.  The keys' cached points are used when every key of every batch is a
    VerifyingKey."""
    eng = engine or default_engine()
    names = {_e.SCALAR_FORMAT: "ScalarFormat", _e.VERIFY: "Verify", _e.NONE: "PointDecompression"}
    out = [None] * len(batches)
    msgs, sigs, keys, off, where = [], [], [], [0], []
    for b, (m, s, k) in enumerate(batches):
        m, s, k = list(m), list(s), list(k)
        if not (len(m) == len(s) == len(k)):
            out[b] = SignatureError("ArrayLength")          # batch.rs:152-165
            continue
        msgs += m; sigs += s; keys += k
        off.append(len(msgs)); where.append(b)
    if not where:
        return out
    pk_points = None
    if keys and all(isinstance(k, VerifyingKey) for k in keys):
        pk_points = _cat([k.point for k in keys], 160)
    st = eng.verify_batch_segments(msgs, sigs, [bytes(k) for k in keys], off, z_mode, pk_points=pk_points)
    for b, c in zip(where, st):
        out[b] = None if c == _e.OK else SignatureError(names[int(c)])
    return out


def x25519_public_keys(secrets, engine=None):
    """PublicKey::from(&StaticSecret | &EphemeralSecret) (x25519-dalek/src/x25519.rs:105-109, :255-259), batched:
    EdwardsPoint::mul_base_clamped(secret).to_montgomery() through the fixed-base tables, not the ladder."""
    eng = engine or default_engine()
    out = eng.x25519_base_batch(_cat(secrets, 32))
    return [out[i].tobytes() for i in range(out.shape[0])]


def verify_each(messages, signatures, verifying_keys, strict=False, engine=None):
    """Per-signature VerifyingKey::verify (verifying.rs:565) or verify_strict (:359): a list with None for
    Ok(()) and a SignatureError for every failing signature."""
    eng = engine or default_engine()
    st = eng.verify_each(list(messages), list(signatures), list(verifying_keys), strict)
    names = {_e.SCALAR_FORMAT: "ScalarFormat", _e.VERIFY: "Verify", _e.NONE: "PointDecompression"}
    return [None if c == _e.OK else SignatureError(names[int(c)]) for c in st]


def verify_each_prehashed(prehashed_messages, signatures, verifying_keys, context=None, strict=False, engine=None):
    """VerifyingKey::verify_prehashed (verifying.rs:284) / verify_prehashed_strict (:424) per signature -- Ed25519ph.  prehashed_messages: hashlib.sha512
    objects (the reference takes a Digest state and finalises it) or their 64-byte digests; context: None (= empty, as in the reference) or up to 255
    bytes, one for the batch.  -> a list with None for Ok(()) and a SignatureError otherwise.  A context beyond 255 bytes raises
    SignatureError("PrehashedContextLength") (the reference debug-asserts on verification and returns that error when signing)."""
    eng = engine or default_engine()
    st = eng.verify_each_prehashed([_digest64(m) for m in prehashed_messages], list(signatures), list(verifying_keys), context or b"", strict)
    if isinstance(st, int):
        raise SignatureError("PrehashedContextLength")
    names = {_e.SCALAR_FORMAT: "ScalarFormat", _e.VERIFY: "Verify", _e.NONE: "PointDecompression"}
    return [None if c == _e.OK else SignatureError(names[int(c)]) for c in st]


def sign_batch_prehashed(secret_keys, prehashed_messages, context=None, engine=None):
    """SigningKey::from_bytes(sk).sign_prehashed(digest, context) for every pair (signing.rs:312 -> :917-976): -> (verifying keys, signatures);
    raises SignatureError("PrehashedContextLength") for a context beyond 255 bytes (signing.rs:931-933)."""
    eng = engine or default_engine()
    r = eng.sign_batch_prehashed(list(secret_keys), [_digest64(m) for m in prehashed_messages], context or b"")
    if isinstance(r, int):
        raise SignatureError("PrehashedContextLength")
    pks, sigs = r
    return [pks[i].tobytes() for i in range(len(secret_keys))], [sigs[i].tobytes() for i in range(len(secret_keys))]


def _digest64(m):
    d = m.digest() if hasattr(m, "digest") else bytes(m)
    if len(d) != 64:
        raise SignatureError("prehashed message: a 512-bit digest is required")
    return d


def sign_batch(secret_keys, messages, engine=None):
    """SigningKey::from_bytes(sk).sign(m) for every pair (signing.rs:878-905): -> (verifying keys, signatures)."""
    eng = engine or default_engine()
    pks, sigs = eng.sign_batch(list(secret_keys), list(messages))
    return [pks[i].tobytes() for i in range(len(messages))], [sigs[i].tobytes() for i in range(len(messages))]


def multiscalar_mul(scalars, points, engine=None):
    """EdwardsPoint::multiscalar_mul (edwards.rs:966-1000), points as CompressedEdwardsY: regular schedule."""
    if len(scalars) != len(points):
        raise AssertionError("multiscalar_mul: scalars and points must have equal length")
    eng = engine or default_engine()
    st, out = eng.msm_consttime(_cat(scalars, 32), _cat(points, 32), _e.FMT_EDWARDS_Y, _e.FMT_EDWARDS_Y)
    return None if st == _e.NONE else out


class VartimeEdwardsPrecomputation:
    """edwards.rs:1037-1076 (VartimePrecomputedMultiscalarMul, traits.rs:304-419); points as CompressedEdwardsY."""

    _fmt = _e.FMT_EDWARDS_Y

    def __init__(self, static_points, engine=None):
        self.eng = engine or default_engine()
        self.h = self.eng.precomp_create(_cat(static_points, 32), self._fmt)

    def __len__(self):
        return self.eng.precomp_len(self.h)

    def is_empty(self):
        return len(self) == 0

    def vartime_mixed_multiscalar_mul(self, static_scalars, dynamic_scalars, dynamic_points):
        if len(dynamic_scalars) != len(dynamic_points):
            raise AssertionError("dynamic scalars and points must have equal length")   # precomputed_straus.rs:87
        st, out = self.eng.precomp_msm_vartime(self.h, _cat(static_scalars, 32), _cat(dynamic_scalars, 32), _cat(dynamic_points, 32),
                                               self._fmt, self._fmt)
        return None if st == _e.NONE else out

    def vartime_multiscalar_mul(self, static_scalars):
        return self.vartime_mixed_multiscalar_mul(static_scalars, [], [])

    def vartime_multiscalar_mul_many(self, rows):
        """[vartime_multiscalar_mul(row)] for every row in ONE call: rows is a list of scalar lists of one length w <= len(self) -> a list of
        32-byte encodings.  The first call builds the handle's comb table (64 KB per static point, Engine.precomp_rows_table_bytes); handles
        of more than engine.PRECOMP_ROWS_MAX_POINTS points are refused (call vartime_multiscalar_mul row by row)."""
        rows = [list(r) for r in rows]
        w = len(rows[0]) if rows else 0
        if any(len(r) != w for r in rows):
            raise AssertionError("vartime_multiscalar_mul_many: every row must have the same number of scalars")
        s = _cat([x for r in rows for x in r], 32).reshape(len(rows), w, 32)
        out = self.eng.precomp_msm_vartime_rows(self.h, s, _e.PRECOMP_ROWS_AUTO, self._fmt)
        return [out[i].tobytes() for i in range(out.shape[0])]

    def vartime_mixed_multiscalar_mul_many(self, rows):
        """[vartime_mixed_multiscalar_mul(*row)] for every row in ONE call: rows is a list of (static_scalars, dynamic_scalars, dynamic_points)
        -> a list with the 32-byte encoding per row, or None where a dynamic point of that row does not decode.  Rows of unequal static width
        are zero-padded to the widest (a zero scalar adds nothing); a row may have at most engine.MSM_SEGMENT_WAVE_MAX dynamic terms (call
        vartime_mixed_multiscalar_mul for a longer one).  The comb table is the one vartime_multiscalar_mul_many builds."""
        rows = [(list(a), list(b), list(c)) for a, b, c in rows]
        if any(len(b) != len(c) for _, b, c in rows):
            raise AssertionError("dynamic scalars and points must have equal length")   # precomputed_straus.rs:87
        w = max([len(a) for a, _, _ in rows], default=0)
        zero = bytes(32)
        ss = _cat([x for a, _, _ in rows for x in a + [zero] * (w - len(a))], 32).reshape(len(rows), w, 32)
        off = np.cumsum([0] + [len(b) for _, b, _ in rows]).astype(np.uint64)
        st, out, ok = self.eng.precomp_msm_vartime_mixed_rows(self.h, ss, _cat([x for _, b, _ in rows for x in b], 32), _cat([x for _, _, c in rows for x in c], 32),
                                                              off, self._fmt, _e.PRECOMP_ROWS_AUTO, self._fmt)
        return [out[i].tobytes() if ok[i] else None for i in range(out.shape[0])]

    def vartime_mixed_multiscalar_mul_folded(self, rows, weights):
        """sum_r weights[r] * vartime_mixed_multiscalar_mul(*rows[r]) as ONE multiscalar mul: rows as for vartime_mixed_multiscalar_mul_many (any
        number of dynamic terms per row), weights one 16-byte (128-bit, as ed25519-dalek/src/batch.rs:207-233 draws them) or 32-byte
        little-endian integer per row -> the 32-byte encoding of the point, or None if a dynamic point does not decode.  The m equations
        "row r sums to the identity" all hold iff (up to the weights' randomness) the result is the identity encoding; to find a bad row,
        run vartime_mixed_multiscalar_mul_many.  Scalars are multiplied by their row's weight mod l on the GPU: exact in the Ristretto group
        and for torsion-free Edwards points (a point with torsion changes the result by a small-order point, as in verify_batch).  No comb
        table is built."""
        rows = [(list(a), list(b), list(c)) for a, b, c in rows]
        if any(len(b) != len(c) for _, b, c in rows):
            raise AssertionError("dynamic scalars and points must have equal length")   # precomputed_straus.rs:87
        w = max([len(a) for a, _, _ in rows], default=0)
        zero = bytes(32)
        ss = _cat([x for a, _, _ in rows for x in a + [zero] * (w - len(a))], 32).reshape(len(rows), w, 32)
        off = np.cumsum([0] + [len(b) for _, b, _ in rows]).astype(np.uint64)
        st, out = self.eng.precomp_msm_vartime_mixed_rows_fold(self.h, ss, _cat([x for _, b, _ in rows for x in b], 32), _cat([x for _, _, c in rows for x in c], 32),
                                                               off, _weights(weights, len(rows)), self._fmt, self._fmt)
        return None if st == _e.NONE else out

    def close(self):
        if self.h:
            self.eng.precomp_destroy(self.h)
            self.h = None


class VartimeRistrettoPrecomputation(VartimeEdwardsPrecomputation):
    """ristretto.rs:1004 (VartimePrecomputedMultiscalarMul for RistrettoPoint): the same precomputation over CompressedRistretto static and
    dynamic points, results as CompressedRistretto."""
    _fmt = _e.FMT_RISTRETTO
