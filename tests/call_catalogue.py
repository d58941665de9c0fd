"""A catalogue of calls on one context, for the sequence tests (tests/test_call_sequences_host.py, tests/test_gpu_call_sequences.py).

A Step is a name, a family, the device inputs it reads (numpy arrays here, uploaded once per process by Bound), a function fn(b, d) that makes
the call on the engine of the Bound b with the device tensors d, and the expected result.  Every expected result comes from the references alone
-- the CPU oracle (oracle/orc.py), the big-integer restatements tests/pyref*.py, Python integers mod l -- never from the engine: `ref` names
the source.  Points are multiples k * B of the basepoint with k known, so what any multiscalar call must return is one orc.ed_mul_base of a
scalar computed with Python integers (the sum-of-squares identity of tests/test_gpu_msm.py is the case points = scalars).

fn returns what the call returned, device tensors included, WITHOUT reading them: the tests decide when the host looks (after the next call,
after a stream synchronisation, after three rounds of queueing).  check(step, raw) then brings everything to the host, applies the step's
`norm` (RAW160 rows to their canonical encodings through the oracle, rows the call declares invalid masked out, records folded by the
library's host arithmetic) and compares with `want`.  A call that must fail with a negative status has want = Raises(part of the message).

The shapes are the smallest that reach each route, found with the host-arithmetic planners (Engine.msm_route, msm_vartime_segments_routes,
verify_batch_segments_plan, batch_transcript_zs_segments_plan, precomp_msm_vartime_rows_plan) and with ffi_chunk_units of csrc/ffi.h restated
below; tests/test_call_sequences_host.py asserts that the routes are really reached, so a boundary that moves fails there.

Enqueue-only or synchronising, by the wording of include/c25519_hip.h ("_dev entry points ... enqueue on the context's HIP stream; those that
return a verdict/point to the host synchronise that stream", and the per-call notes).  The first column holds glob patterns of step names;
tests/test_call_sequences_host.py checks that every step falls under exactly one row and carries that row's flag:

  step (prefix)                                    entry point                                              host visit
  -----------------------------------------------  -------------------------------------------------------  ------------------------------------------
  fixed.mul_base_ct, fixed.mul_base_vartime        c25519_mul_base_batch[_vartime]_dev                      enqueue only
  fixed.x25519, fixed.x25519_base                  c25519_x25519[_base]_batch_dev                           enqueue only
  fixed.decompress_none                            c25519_decompress_batch_dev                              synchronises (returns NONE)
  fixed.compress                                   c25519_compress_batch_dev                                enqueue only
  fixed.mul_batch_none, fixed.double_base_none     c25519_mul_batch_dev, c25519_double_base_batch_dev       enqueue only (ok[] stays on the device)
  fixed.montgomery_mul                             c25519_montgomery_mul_batch_dev                          enqueue only
  fixed.order_checks                               c25519_point_order_checks_batch_dev                      enqueue only
  fixed.scalar_invert                              c25519_scalar_invert_batch (host pointers)               synchronises
  fixed.mul_table                                  c25519_mul_table_batch_dev                               enqueue only
  msm.*.ok, msm.*.none, msm.*.bit255               c25519_msm_vartime_dev                                   synchronises (out is a host pointer)
  msm.partial_record.*                             c25519_msm_partial_record_dev                            enqueue only ("only ENQUEUES")
  msm.consttime                                    c25519_msm_consttime (host pointers)                     synchronises
  verify.*                                         ed25519_verify_batch_keys_dev                            synchronises (returns the verdict)
  chain.*                                          ed25519_batch_hram_dev -> ed25519_batch_transcript_zs_   enqueue only, all three ("never visits the host")
                                                   segments_dev -> ed25519_verify_batch_record_dev
  seg.verify.*                                     ed25519_verify_batch_segments_dev                        synchronises (msg_off verdict; host sponge)
  seg.msm.*                                        c25519_msm_vartime_segments_dev                          synchronises once, at the end
  precomp.single                                   c25519_precomp_msm_vartime (host pointers)               synchronises
  precomp.rows_*, precomp.mixed_rows               c25519_precomp_msm_vartime_[mixed_]rows_dev              synchronise once, at the end
  precomp.fold                                     c25519_precomp_msm_vartime_mixed_rows_fold_dev           synchronises (out is a host pointer)
  group.add_raw, group.sum_segments, group.eq      c25519_point_{add_batch,sum_segments,eq_batch}_dev RAW   enqueue only ("with RAW160 input they do not")
  group.add_compressed_none                        c25519_point_add_batch_dev, compressed input             synchronises (reads the verdict)
  hash.ristretto, hash.edwards, hash.*_bad_off     c25519_{ristretto_hash_from_bytes,edwards_hash_to_       synchronise ("read that verdict back")
                                                   curve}_batch_dev
  hash.lizard_encode, hash.lizard_decode           c25519_ristretto_lizard_{en,de}code_sha256_batch_dev     enqueue only
  secret.keygen                                    ed25519_keygen_batch_dev                                 enqueue only
  secret.sign, secret.sign_prehashed               ed25519_sign_batch[_prehashed]_dev                       synchronise (msg_off verdict)
  secret.verify_each                               ed25519_verify_each_dev                                  enqueue only
  host.*                                           the host-pointer twins                                   synchronise (the results are on the host)
"""
import os
import re

import numpy as np

import pyref_finish
import pyref_h2c
import pyref_lizard
import pyref_montgomery
import util

L = util.L
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "curve25519-dalek_amd", "csrc")
OK, NONE, SCALAR_FORMAT, VERIFY = 0, 1, 2, 3
ED, RIS, RAW = 0, 1, 2
Z_TRANSCRIPT, Z_DEVICE = 0, 1
THREADS = min(16, os.cpu_count() or 1)
BAD_POINT = (2).to_bytes(32, "little")                       # y = 2 is not on the curve (asserted against the oracle by the host test)
MSG_LEN = 40
FAMILIES = ("fixed", "msm", "verify", "chain", "seg", "precomp", "group", "hash", "secret", "host")


def i2b(x, n=32):
    return int(x).to_bytes(n, "little")


def b2i(b):
    return int.from_bytes(bytes(b), "little")


def rows(a):
    return [bytes(r) for r in a]


def arr(items, width=32):
    return np.frombuffer(b"".join(bytes(x) for x in items), np.uint8).reshape(-1, width).copy() if len(items) else np.zeros((0, width), np.uint8)


def offsets(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int64)


class Raises:
    """the expected result of a call that must fail with a negative status: EngineError whose message contains `part`"""

    def __init__(self, part):
        self.part = part

    def __repr__(self):
        return "Raises(%r)" % self.part


class Raised:
    """what Bound.run returns for a call that raised EngineError"""

    def __init__(self, message):
        self.message = message

    def __repr__(self):
        return "Raised(%r)" % self.message


class Step:
    def __init__(self, name, fn, want, ref, inputs=None, norm=None, enqueue_only=False, needs=(), **meta):
        self.name, self.fn, self.want, self.ref = name, fn, want, ref
        self.family = name.split(".")[0]
        assert self.family in FAMILIES, name
        self.inputs = dict(inputs or {})
        self.norm = norm
        self.enqueue_only = enqueue_only
        self.needs = tuple(needs)                            # per-engine handles: "basetable", "precomp"
        self.meta = meta                                     # what the host test checks the shape and the failing variant by

    def __repr__(self):
        return "Step(%s)" % self.name


# ---- running and checking ---------------------------------------------------------------------------------------------------------
_UPLOADED = {}                                               # id(numpy array) -> (the array, its CUDA tensor): inputs shared by steps go up once per process


def upload(a):
    import torch
    hit = _UPLOADED.get(id(a))
    if hit is None:
        hit = _UPLOADED[id(a)] = (a, torch.from_numpy(a).cuda())
    return hit[1]


class Bound:
    """an engine with the per-engine handles of the catalogue (created on first use) and the device inputs of its steps"""

    def __init__(self, eng, cat):
        self.eng, self.cat = eng, cat
        self._handles = {}

    def handle(self, what):
        if what not in self._handles:
            if what == "basetable":
                self._handles[what] = self.eng.basetable_create(self.cat.table_point, in_fmt=ED)
            else:
                self._handles[what] = self.eng.precomp_create(self.cat.static_enc, in_fmt=ED)
        return self._handles[what]

    def dev(self, step):
        return {k: upload(v) for k, v in step.inputs.items()}

    def prepare(self, steps):
        """everything a later run() would otherwise fetch or build with a host visit: device inputs and handles"""
        for s in steps:
            self.dev(s)
            for h in s.needs:
                self.handle(h)

    def run(self, step, dev=None):
        """make the call; -> what it returned (device tensors unread) or Raised"""
        import curve25519_dalek_amd as pkg
        for h in step.needs:
            self.handle(h)
        d = self.dev(step) if dev is None else dev
        try:
            return step.fn(self, d)
        except pkg.EngineError as e:
            return Raised(str(e))

    def close(self):
        for what, h in self._handles.items():
            (self.eng.basetable_destroy if what == "basetable" else self.eng.precomp_destroy)(h)
        self._handles = {}


def tohost(x):
    if hasattr(x, "is_cuda"):
        return x.cpu().numpy()
    if isinstance(x, (tuple, list)):
        return tuple(tohost(v) for v in x)
    return x


def same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a, b))
    if isinstance(a, (tuple, list)) or isinstance(b, (tuple, list)):
        return isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return type(a) == type(b) and a == b


def describe(v):
    if isinstance(v, np.ndarray):
        return "array%s:%s" % (v.shape, bytes(v.reshape(-1)[:48]).hex())
    if isinstance(v, (tuple, list)):
        return "(" + ", ".join(describe(x) for x in v) + ")"
    if isinstance(v, bytes):
        return v[:48].hex()
    return repr(v)


def first_difference(a, b):
    if isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.shape == b.shape and a.ndim >= 1 and a.shape[0]:
        bad = np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0]
        return "rows %s of %d differ" % (bad[:8].tolist(), a.shape[0]) if bad.size else ""
    if isinstance(a, tuple) and isinstance(b, tuple) and len(a) == len(b):
        return "; ".join("[%d] %s" % (i, first_difference(x, y)) for i, (x, y) in enumerate(zip(a, b)) if not same(x, y))
    return ""


def check(step, raw):
    """-> "" if what the call returned equals the reference, else what differs.  Reads the device tensors of `raw` (a host visit)."""
    if isinstance(step.want, Raises):
        if isinstance(raw, Raised) and step.want.part in raw.message:
            return ""
        return "%s: expected an EngineError with %r, got %s" % (step.name, step.want.part, describe(tohost(raw)) if not isinstance(raw, Raised) else raw)
    if isinstance(raw, Raised):
        return "%s: the call failed: %s" % (step.name, raw.message)
    got = tohost(raw)
    if step.norm is not None:
        got = step.norm(got)
    if same(got, step.want):
        return ""
    return "%s: differs from %s: %s\n    got  %s\n    want %s" % (step.name, step.ref, first_difference(got, step.want), describe(got), describe(step.want))


# ---- csrc/ffi.h, restated ---------------------------------------------------------------------------------------------------------
def ffi_maxch():
    m = re.search(r"static const int FFI_MAXCH = (\d+);", open(os.path.join(CSRC, "ctx.h")).read())
    return int(m.group(1))


def ffi_chunk_units(n, min_units):
    """csrc/ffi.h ffi_chunk_units: at most FFI_MAXCH chunks of at least min_units units, a multiple of 1024"""
    if n <= min_units:
        return n if n else 1
    nch = min(n // min_units, ffi_maxch())
    c = (n + nch - 1) // nch
    return (c + 1023) & ~1023


def ffi_chunks(n, min_units):
    c = ffi_chunk_units(n, min_units)
    return (n + c - 1) // c


def ffi_min_units():
    """the min_units the host twins of mul_base_batch and x25519_batch hand to ffi_chunk_units, read off their source"""
    src = open(os.path.join(CSRC, "capi.hip")).read()
    mb = re.search(r"static int32_t mul_base_host\(.*?ffi_twin\(ctx, n, 1u << (\d+),", src, re.S)
    xh = re.search(r"static int32_t x25519_host\(.*?ffi_chunk_units\(n, 1u << (\d+)\)", src, re.S)
    return 1 << int(mb.group(1)), 1 << int(xh.group(1))


def smallest(pred, start=1, limit=1 << 26):
    """the smallest n >= start with pred(n), for a predicate that is false below a threshold and true from it on"""
    hi = start
    while not pred(hi):
        hi *= 2
        assert hi <= limit
    lo = hi // 2 if hi > start else start - 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(mid):
            hi = mid
        else:
            lo = mid
    return hi


# ---- the catalogue ----------------------------------------------------------------------------------------------------------------
class Catalogue:
    def __init__(self, orc):
        import curve25519_dalek_amd as pkg
        self.orc, self.pkg, self.E = orc, pkg, pkg.Engine
        self.steps = []
        self.PB = lambda v: orc.ed_compress(orc.ed_mul_base(i2b(v % L)))                 # the encoding of v * B
        self._shared()
        self._fixed()
        self._msm()
        self._verify()
        self._chain()
        self._segments()
        self._precomp()
        self._group()
        self._hash()
        self._secret()
        self._host()
        names = [s.name for s in self.steps]
        assert len(set(names)) == len(names)
        self.by_name = {s.name: s for s in self.steps}

    def add(self, *a, **k):
        self.steps.append(Step(*a, **k))

    def family(self, f):
        return [s for s in self.steps if s.family == f]

    def enqueue_only(self):
        return [s for s in self.steps if s.enqueue_only]

    def raw_of(self, enc):
        """RAW160 of compressed points through the oracle's decompression"""
        return arr([self.orc.ed_decompress(bytes(e)) for e in enc], 160)

    def compress_rows(self, raw):
        return arr([self.orc.ed_compress(bytes(r)) for r in raw], 32)

    def mulB(self, ks):
        """encodings of k * B for Python integers k"""
        return self.orc.mul_base_compress_batch(arr([i2b(k % L) for k in ks]), threads=THREADS) if len(ks) else np.zeros((0, 32), np.uint8)

    # -- inputs several families share ------------------------------------------------------------------------------------------------
    def _shared(self):
        orc, E = self.orc, self.E
        self.msm_n = {p: smallest(lambda n, p=p: E.msm_route(0, n, ED)["path"] == p) for p in ("small", "mid", "pipeline")}
        self.verify_n = {p: smallest(lambda n, p=p: E.msm_route(1, n)["path"] == p) for p in ("small", "mid", "pipeline")}
        npts = self.msm_n["pipeline"]
        self.x = util.rand_scalars(4100, npts)                                              # points x_i * B: the sum-of-squares identity
        self.X = [b2i(r) for r in self.x]
        self.enc = orc.mul_base_compress_batch(self.x, threads=THREADS)
        self.raw = self.raw_of(self.enc[:160])                                              # the first of them as RAW160
        nsig = self.verify_n["pipeline"]
        self.seeds = util.rand_bytes(4101, nsig)
        self.msgs = util.rand_bytes(4102, nsig, MSG_LEN)
        self.pks, self.sigs = orc.ed25519_keygen_sign_batch(self.seeds, self.msgs, threads=THREADS)
        self.static_k = [b2i(r) for r in util.rand_scalars(4103, 12)]                       # the precomputation handle: 12 static points
        self.static_enc = self.mulB(self.static_k)
        self.table_k = b2i(util.rand_scalars(4104, 1)[0])
        self.table_point = bytes(self.mulB([self.table_k])[0])

    # -- fixed base and per-item ------------------------------------------------------------------------------------------------------
    def _fixed(self):
        orc, add = self.orc, self.add
        n = 130
        for name, seed, call in (("fixed.mul_base_ct", 4110, "mul_base_batch_t"), ("fixed.mul_base_vartime", 4111, "mul_base_batch_vartime_t")):
            s = util.rand_scalars(seed, n)
            s[0], s[1], s[2] = arr([i2b(0)])[0], arr([i2b(1)])[0], arr([i2b(L - 1)])[0]
            add(name, lambda b, d, call=call: getattr(b.eng, call)(d["s"]), orc.mul_base_compress_batch(s), "orc.mul_base_compress_batch",
                inputs={"s": s}, enqueue_only=True)
        k, u = util.rand_bytes(4112, n), util.rand_bytes(4113, n)
        add("fixed.x25519", lambda b, d: b.eng.x25519_batch_t(d["k"], d["u"]), orc.x25519_batch(k, u), "orc.x25519_batch", inputs={"k": k, "u": u}, enqueue_only=True)
        nine = np.zeros((n, 32), np.uint8); nine[:, 0] = 9
        add("fixed.x25519_base", lambda b, d: b.eng.x25519_base_batch_t(d["k"]), orc.x25519_batch(k, nine), "orc.x25519_batch(k, 9)", inputs={"k": k}, enqueue_only=True)

        enc = self.enc[:n].copy(); enc[77] = arr([BAD_POINT])[0]
        okv = orc.ed_decompress_ok_batch(enc)

        def norm_dec(g, enc=enc):
            st, pts, ok = g                                  # the points of the rows that decode, as the oracle encodes them
            return st, arr([orc.ed_compress(bytes(pts[i])) if ok[i] else bytes(32) for i in range(len(ok))]), ok
        add("fixed.decompress_none", lambda b, d: b.eng.decompress_batch_t(d["enc"]), (NONE, np.where(okv[:, None] == 1, enc, 0).astype(np.uint8), okv),
            "orc.ed_decompress_ok_batch, orc.ed_compress", inputs={"enc": enc}, norm=norm_dec, bad_rows=[77], status=NONE)
        add("fixed.compress", lambda b, d: b.eng.compress_batch_t(d["raw"]), self.enc[:n].copy(), "orc.ed_decompress of orc.mul_base_compress_batch",
            inputs={"raw": self.raw[:n].copy()}, enqueue_only=True)

        s = util.rand_scalars(4114, n); S = [b2i(r) for r in s]
        mask = lambda g: (np.where(g[1][:, None] == 1, g[0], 0).astype(np.uint8), g[1])
        add("fixed.mul_batch_none", lambda b, d: b.eng.mul_batch_t(d["s"], d["enc"], in_fmt=ED, out_fmt=ED),
            (np.where(okv[:, None] == 1, self.mulB([S[i] * self.X[i] for i in range(n)]), 0).astype(np.uint8), okv), "orc.mul_base_compress_batch(s_i x_i mod l)",
            inputs={"s": s, "enc": enc}, norm=mask, enqueue_only=True, bad_rows=[77])
        t = util.rand_scalars(4115, n); T = [b2i(r) for r in t]
        add("fixed.double_base_none", lambda b, d: b.eng.double_base_batch_t(d["s"], d["enc"], d["t"], in_fmt=ED, out_fmt=ED),
            (np.where(okv[:, None] == 1, self.mulB([S[i] * self.X[i] + T[i] for i in range(n)]), 0).astype(np.uint8), okv),
            "orc.mul_base_compress_batch(s_i x_i + t_i mod l)", inputs={"s": s, "enc": enc, "t": t}, norm=mask, enqueue_only=True, bad_rows=[77])

        km, um = util.rand_bytes(4116, 20), util.rand_bytes(4117, 20)
        add("fixed.montgomery_mul", lambda b, d: b.eng.montgomery_mul_batch_t(d["k"], d["u"]), arr([pyref_montgomery.mul(bytes(um[i]), bytes(km[i])) for i in range(20)]),
            "pyref_montgomery.mul", inputs={"k": km, "u": um}, enqueue_only=True)

        t8 = pyref_finish.torsion8()
        pts = arr(rows(self.enc[:4]) + [i2b(1)] + [pyref_finish.compress(t8[j]) for j in (1, 2, 4)] + [BAD_POINT] + rows(self.enc[4:8]))

        def flags(e):
            p = orc.ed_decompress(bytes(e))
            return 0 if p is None else 1 | (2 if orc.ed_is_small_order(p) else 0) | (4 if orc.ed_is_torsion_free(p) else 0)
        add("fixed.order_checks", lambda b, d: b.eng.point_order_checks_t(d["p"], in_fmt=ED), np.array([flags(e) for e in pts], np.uint8),
            "orc.ed_is_small_order, orc.ed_is_torsion_free", inputs={"p": pts}, enqueue_only=True)

        v = util.rand_scalars(4118, 20); v[:, 0] |= 1; V = [b2i(r) for r in v]
        inv = [pow(x, -1, L) for x in V]
        prod = 1
        for x in inv:
            prod = prod * x % L
        add("fixed.scalar_invert", lambda b, d: b.eng.scalar_invert_batch(v), (arr([i2b(x) for x in inv]), i2b(prod)), "pow(v, -1, l): Python integers mod l")
        st = util.rand_scalars(4119, 70)
        add("fixed.mul_table", lambda b, d: b.eng.mul_table_batch_t(b.handle("basetable"), d["s"]), self.mulB([b2i(r) * self.table_k for r in st]),
            "orc.mul_base_compress_batch(s_i k mod l)", inputs={"s": st}, enqueue_only=True, needs=("basetable",))

    # -- msm_vartime ------------------------------------------------------------------------------------------------------------------
    def _msm(self):
        orc, add = self.orc, self.add
        sizes = dict(self.msm_n); sizes["small300"] = 300                                   # (one small-path call of more than one term as well)
        for path, n in sizes.items():
            x, enc = np.ascontiguousarray(self.x[:n]), np.ascontiguousarray(self.enc[:n])
            want = self.PB(sum(v * v for v in self.X[:n]))
            route = path.rstrip("0123456789")
            run = lambda b, d: b.eng.msm_vartime_t(d["x"], d["enc"], in_fmt=ED, out_fmt=ED)
            add("msm.%s.ok" % path, run, (OK, want), "orc.ed_mul_base(sum x_i^2 mod l)", inputs={"x": x, "enc": enc}, route=route, n=n, status=OK)
            bad = enc.copy(); bad[n // 3] = arr([BAD_POINT])[0]
            add("msm.%s.none" % path, run, (NONE,), "orc.ed_decompress(y = 2) is None", inputs={"x": x, "enc": bad}, norm=lambda g: (g[0],), route=route, n=n,
                status=NONE, bad_rows=[n // 3])
            hi = x.copy(); hi[(2 * n) // 3, 31] |= 0x80
            add("msm.%s.bit255" % path, run, Raises("bit 255"), "Scalar invariant #1: a scalar with bit 255 set is refused", inputs={"x": hi, "enc": enc}, route=route, n=n)

        def fold(g):
            st, out = self.pkg.engine.fold_partial_records(g[None, :], out_fmt=ED)
            return st, out
        for path in ("small300", "mid"):
            n = sizes[path]
            add("msm.partial_record.%s" % path, lambda b, d: b.eng.msm_partial_record_t(d["x"], d["enc"], in_fmt=ED), (OK, self.PB(sum(v * v for v in self.X[:n]))),
                "orc.ed_mul_base(sum x_i^2 mod l)", inputs={"x": np.ascontiguousarray(self.x[:n]), "enc": np.ascontiguousarray(self.enc[:n])}, norm=fold, enqueue_only=True,
                route=path.rstrip("0123456789"), n=n)
        s = util.rand_scalars(4120, 17)
        add("msm.consttime", lambda b, d: b.eng.msm_consttime(s, self.raw[:17], in_fmt=RAW, out_fmt=ED), (OK, self.PB(sum(b2i(s[i]) * self.X[i] for i in range(17)))),
            "orc.ed_mul_base(sum s_i x_i mod l)")

    # -- verify_batch -----------------------------------------------------------------------------------------------------------------
    def batch(self, n, variant="honest", lo=0):
        """signatures [lo, lo + n) of the shared batch with one defect in the middle -> (msgs blob, offsets, sigs, pks, index of the defect)"""
        msgs, sigs, pks = self.msgs[lo:lo + n].reshape(-1).copy(), self.sigs[lo:lo + n].copy(), self.pks[lo:lo + n].copy()
        j = n // 2
        if variant == "forged":
            sigs[j, 3] ^= 1                                                                  # a bit of R
        elif variant == "noncanonical":
            sigs[j, 32:] = np.frombuffer(i2b(b2i(sigs[j, 32:]) + L), np.uint8)              # s + l: the same residue, not canonical
        elif variant == "badkey":
            pks[j] = arr([BAD_POINT])[0]
        else:
            assert variant == "honest"
        return msgs, offsets([MSG_LEN] * n), sigs, pks, j

    def verdicts(self, msgs, off, sigs, pks):
        """-> (the oracle's verify_batch status, its per-signature statuses)"""
        n = sigs.shape[0]
        M = [bytes(msgs[int(off[i]):int(off[i + 1])]) for i in range(n)]
        S, K = rows(sigs), rows(pks)
        return self.orc.ed25519_verify_batch(M, S, K), [self.orc.ed25519_verify(K[i], M[i], S[i]) for i in range(n)]

    def _verify(self):
        orc, add = self.orc, self.add
        expect = {"honest": OK, "forged": VERIFY, "noncanonical": SCALAR_FORMAT, "badkey": NONE}
        sizes = [("1", 1), ("64", 64), ("mid", self.verify_n["mid"])]
        self.verify_sizes = dict(sizes)
        for label, n in sizes:
            for variant in expect:
                msgs, off, sigs, pks, j = self.batch(n, variant)
                want, each = self.verdicts(msgs, off, sigs, pks)
                for z in (Z_TRANSCRIPT, Z_DEVICE):
                    add("verify.%s.%s.z%d" % (label, variant, z), lambda b, d, z=z: b.eng.verify_batch_t(d["msgs"], d["off"], d["sigs"], d["pks"], z), want,
                        "orc.ed25519_verify_batch", inputs={"msgs": msgs, "off": off, "sigs": sigs, "pks": pks}, n=n, variant=variant, defect=j, each=each,
                        status=expect[variant], route=self.E.msm_route(1, n)["path"])
        for variant in ("honest", "forged"):                                                # VerifyingKey's cached points given
            msgs, off, sigs, pks, j = self.batch(64, variant)
            want, each = self.verdicts(msgs, off, sigs, pks)
            pts = self.raw_of(pks)
            for z in (Z_TRANSCRIPT, Z_DEVICE):
                add("verify.64.%s_pk_points.z%d" % (variant, z), lambda b, d, z=z: b.eng.verify_batch_t(d["msgs"], d["off"], d["sigs"], d["pks"], z, pk_points=d["pts"]),
                    want, "orc.ed25519_verify_batch", inputs={"msgs": msgs, "off": off, "sigs": sigs, "pks": pks, "pts": pts}, n=64, variant=variant, defect=j, each=each,
                    status=expect[variant], route="small")
        msgs, off, sigs, pks, _ = self.batch(64)
        bad = off.copy(); bad[10] = bad[12]
        for z in (Z_TRANSCRIPT, Z_DEVICE):
            add("verify.64.bad_off.z%d" % z, lambda b, d, z=z: b.eng.verify_batch_t(d["msgs"], d["off"], d["sigs"], d["pks"], z), Raises("msg_off"),
                "msg_off must be non-decreasing (include/c25519_hip.h)", inputs={"msgs": msgs, "off": bad, "sigs": sigs, "pks": pks}, n=64, route="small")
        n = self.verify_n["pipeline"]                                                       # the largest call of the family: the bucket pipeline
        want = orc.ed25519_verify_batch_mt_np(self.msgs[:n], MSG_LEN, self.sigs[:n], self.pks[:n], threads=THREADS)
        add("verify.pipeline.honest.z1", lambda b, d: b.eng.verify_batch_t(d["msgs"], d["off"], d["sigs"], d["pks"], Z_DEVICE), want, "orc.ed25519_verify_batch_mt_np",
            inputs={"msgs": self.msgs[:n].reshape(-1), "off": offsets([MSG_LEN] * n), "sigs": self.sigs[:n], "pks": self.pks[:n]}, n=n, variant="honest", status=OK,
            route=self.E.msm_route(1, n)["path"])

    # -- the enqueue-only chain ------------------------------------------------------------------------------------------------------
    def _chain(self):
        orc, add = self.orc, self.add
        n = 64
        for variant, status in (("honest", OK), ("forged", VERIFY)):
            msgs, off, sigs, pks, j = self.batch(n, variant, lo=100)
            want, each = self.verdicts(msgs, off, sigs, pks)
            hram = [orc.sha512(bytes(sigs[i, :32]) + bytes(pks[i]) + bytes(msgs[int(off[i]):int(off[i + 1])])) for i in range(n)]
            zs = arr(orc.batch_transcript_zs(hram, [bytes(sigs[i, 32:]) for i in range(n)]), 16)

            def run(b, d):
                h = b.eng.batch_hram_t(d["msgs"], d["off"], d["sigs"], d["pks"])
                z = b.eng.batch_transcript_zs_segments_t(h, d["sigs"], [0, n])
                return z, b.eng.verify_batch_record_t(d["sigs"], d["pks"], h, z)
            add("chain.%s" % variant, run, (zs, want), "orc.batch_transcript_zs over orc.sha512(R || A || M), orc.ed25519_verify_batch",
                inputs={"msgs": msgs, "off": off, "sigs": sigs, "pks": pks}, norm=lambda g: (g[0], self.pkg.engine.fold_verify_records(g[1][None, :])), enqueue_only=True,
                n=n, variant=variant, defect=j, each=each, status=status)

    # -- segmented calls ---------------------------------------------------------------------------------------------------------------
    def _segments(self):
        orc, add = self.orc, self.add
        lens = [0, 1, 17, 300]
        self.verify_seg_off = off = offsets(lens)
        n = int(off[-1])
        msgs, moff, sigs, pks, _ = self.batch(n, lo=300)
        poisoned = 2
        sigs[int(off[poisoned]) + 5, 3] ^= 1
        want, each = [], []
        for s in range(len(lens)):
            a, e = int(off[s]), int(off[s + 1])
            st, ea = self.verdicts(msgs[a * MSG_LEN:e * MSG_LEN], offsets([MSG_LEN] * (e - a)), sigs[a:e], pks[a:e])
            want.append(st); each.append(ea)
        for z in (Z_TRANSCRIPT, Z_DEVICE):
            add("seg.verify.z%d" % z, lambda b, d, z=z, off=off: b.eng.verify_batch_segments_t(d["msgs"], d["off"], d["sigs"], d["pks"], off, z), np.array(want, np.uint8),
                "orc.ed25519_verify_batch per segment", inputs={"msgs": msgs, "off": moff, "sigs": sigs, "pks": pks}, seg_off=off, poisoned=poisoned, each=each)

        lens = [0, 1, 64, 65, 2049]
        self.msm_seg_off = off = offsets(lens)
        n = int(off[-1])
        s = util.rand_scalars(4130, n); S = [b2i(r) for r in s]
        sums = self.mulB([sum(S[i] * self.X[i] for i in range(int(off[k]), int(off[k + 1]))) for k in range(len(lens))])
        enc = np.ascontiguousarray(self.enc[:n])
        mask = lambda g: (g[0], np.where(g[2][:, None] == 1, g[1], 0).astype(np.uint8), g[2])
        run = lambda b, d, off=off: b.eng.msm_vartime_segments_t(d["s"], d["enc"], off, in_fmt=ED, out_fmt=ED)
        add("seg.msm.ok", run, (OK, sums, np.ones(len(lens), np.uint8)), "orc.mul_base_compress_batch(sum s_i x_i mod l per segment)", inputs={"s": s, "enc": enc}, norm=mask,
            seg_off=off, status=OK)
        poisoned = 3
        bad = enc.copy(); bad[int(off[poisoned]) + 40] = arr([BAD_POINT])[0]
        okv = np.ones(len(lens), np.uint8); okv[poisoned] = 0
        add("seg.msm.none", run, (NONE, np.where(okv[:, None] == 1, sums, 0).astype(np.uint8), okv), "orc.mul_base_compress_batch per segment; orc.ed_decompress(y = 2) is None",
            inputs={"s": s, "enc": bad}, norm=mask, seg_off=off, status=NONE, poisoned=poisoned)

    # -- precomputed static points -----------------------------------------------------------------------------------------------------
    def _precomp(self):
        add, E, K = self.add, self.E, self.static_k
        w = len(K)
        ss = util.rand_scalars(4140, w); ds = util.rand_scalars(4141, 5)
        val = sum(b2i(ss[j]) * K[j] for j in range(w)) + sum(b2i(ds[i]) * self.X[i] for i in range(5))
        dp = np.ascontiguousarray(self.enc[:5])
        add("precomp.single", lambda b, d: b.eng.precomp_msm_vartime(b.handle("precomp"), ss, ds, dp, in_fmt=ED, out_fmt=ED), (OK, self.PB(val)),
            "orc.ed_mul_base(sum s_j k_j + sum d_i x_i mod l)", needs=("precomp",))
        lane_m = smallest(lambda m: E.precomp_msm_vartime_rows_plan(m, 2)[0] == self.pkg.engine.PRECOMP_ROWS_LANE)
        for label, m, wr in (("lane", lane_m, 2), ("wave", 5, w)):
            sc = util.rand_scalars(4142 + m, m * wr).reshape(m, wr, 32)
            A = [[b2i(sc[r, j]) for j in range(wr)] for r in range(m)]
            add("precomp.rows_%s" % label, lambda b, d: b.eng.precomp_msm_vartime_rows_t(b.handle("precomp"), d["sc"]),
                self.mulB([sum(A[r][j] * K[j] for j in range(wr)) for r in range(m)]), "orc.mul_base_compress_batch(sum s_rj k_j mod l)", inputs={"sc": sc},
                needs=("precomp",), m=m, w=wr)
        m, wr, lens = 6, 3, [0, 1, 2, 3, 1, 0]
        doff = offsets(lens)
        nd = int(doff[-1])
        sc = util.rand_scalars(4150, m * wr).reshape(m, wr, 32); dsc = util.rand_scalars(4151, nd); dpt = np.ascontiguousarray(self.enc[20:20 + nd])
        row = [sum(b2i(sc[r, j]) * K[j] for j in range(wr)) + sum(b2i(dsc[i]) * self.X[20 + i] for i in range(int(doff[r]), int(doff[r + 1]))) for r in range(m)]
        add("precomp.mixed_rows", lambda b, d: b.eng.precomp_msm_vartime_mixed_rows_t(b.handle("precomp"), d["sc"], d["ds"], d["dp"], doff, in_fmt=ED, out_fmt=ED),
            (OK, self.mulB(row), np.ones(m, np.uint8)), "orc.mul_base_compress_batch(row sums mod l)", inputs={"sc": sc, "ds": dsc, "dp": dpt}, needs=("precomp",), m=m, w=wr,
            dyn_off=doff)
        wt = util.rand_bytes(4152, m, 16)
        add("precomp.fold", lambda b, d: b.eng.precomp_msm_vartime_mixed_rows_fold_t(b.handle("precomp"), d["sc"], d["ds"], d["dp"], doff, d["wt"], in_fmt=ED, out_fmt=ED),
            (OK, self.PB(sum(b2i(wt[r]) * row[r] for r in range(m)))), "orc.ed_mul_base(sum c_r row_r mod l)", inputs={"sc": sc, "ds": dsc, "dp": dpt, "wt": wt},
            needs=("precomp",), m=m, w=wr, dyn_off=doff)

    # -- the group law -----------------------------------------------------------------------------------------------------------------
    def _group(self):
        add, X = self.add, self.X
        n = 70
        p, q = self.raw[:n].copy(), self.raw[n:2 * n].copy()
        canon = lambda g: (g[0], self.compress_rows(g[1]), g[2])
        ones = np.ones(n, np.uint8)
        add("group.add_raw", lambda b, d: b.eng.point_add_batch_t(d["p"], d["q"], in_fmt=RAW, out_fmt=RAW), (OK, self.mulB([X[i] + X[n + i] for i in range(n)]), ones),
            "orc.mul_base_compress_batch(x_i + x_j mod l), orc.ed_compress", inputs={"p": p, "q": q}, norm=canon, enqueue_only=True)
        pe, qe = self.enc[:n].copy(), self.enc[n:2 * n].copy()
        qe[31] = arr([BAD_POINT])[0]
        okv = ones.copy(); okv[31] = 0
        add("group.add_compressed_none", lambda b, d: b.eng.point_add_batch_t(d["p"], d["q"], in_fmt=ED, out_fmt=ED),
            (NONE, np.where(okv[:, None] == 1, self.mulB([X[i] + X[n + i] for i in range(n)]), 0).astype(np.uint8), okv), "orc.mul_base_compress_batch(x_i + x_j mod l)",
            inputs={"p": pe, "q": qe}, norm=lambda g: (g[0], np.where(g[2][:, None] == 1, g[1], 0).astype(np.uint8), g[2]), status=NONE, bad_rows=[31])
        soff = offsets([0, 1, 32, 37])
        add("group.sum_segments", lambda b, d: b.eng.point_sum_segments_t(d["p"], d["off"], in_fmt=RAW, out_fmt=RAW),
            (OK, self.mulB([sum(X[int(soff[k]):int(soff[k + 1])]) for k in range(4)]), np.ones(4, np.uint8)), "orc.mul_base_compress_batch(segment sums mod l), orc.ed_compress",
            inputs={"p": p, "off": soff}, norm=canon, enqueue_only=True)
        q2 = q.copy(); q2[::2] = p[::2]
        add("group.eq", lambda b, d: b.eng.point_eq_batch_t(d["p"], d["q"], in_fmt=RAW, group=ED), (OK, (np.arange(n) % 2 == 0).astype(np.uint8), ones),
            "x_i == x_j mod l", inputs={"p": p, "q": q2}, enqueue_only=True)

    # -- hashing to the group and Lizard ------------------------------------------------------------------------------------------------
    def _hash(self):
        add = self.add
        msgs = [b"", b"a", bytes(range(63)), bytes(range(64)), bytes(range(200))]
        blob = np.frombuffer(b"".join(msgs), np.uint8).copy()
        off = offsets([len(m) for m in msgs])
        bad = off.copy(); bad[2] = bad[4]
        dst = b"QUUX-V01-CS02-with-edwards25519_XMD:SHA-512_ELL2_RO_"
        add("hash.ristretto", lambda b, d: b.eng.ristretto_hash_from_bytes_batch_t(d["blob"], d["off"]), arr([pyref_h2c.ristretto_hash_from_bytes(m) for m in msgs]),
            "pyref_h2c.ristretto_hash_from_bytes", inputs={"blob": blob, "off": off})
        add("hash.edwards", lambda b, d: b.eng.edwards_hash_to_curve_batch_t(d["blob"], d["off"], dst),
            arr([pyref_h2c.edwards_compress(pyref_h2c.edwards_hash_to_curve(m, dst)) for m in msgs]), "pyref_h2c.edwards_hash_to_curve", inputs={"blob": blob, "off": off})
        add("hash.ristretto_bad_off", lambda b, d: b.eng.ristretto_hash_from_bytes_batch_t(d["blob"], d["off"]), Raises("msg_off"),
            "msg_off must be non-decreasing (include/c25519_hip.h)", inputs={"blob": blob, "off": bad})
        add("hash.edwards_bad_off", lambda b, d: b.eng.edwards_hash_to_curve_batch_t(d["blob"], d["off"], dst), Raises("msg_off"),
            "msg_off must be non-decreasing (include/c25519_hip.h)", inputs={"blob": blob, "off": bad})
        data = util.rand_bytes(4160, 9, 16)
        enc = [pyref_lizard.lizard_encode(bytes(r)) for r in data]
        add("hash.lizard_encode", lambda b, d: b.eng.ristretto_lizard_encode_batch_t(d["data"]), arr(enc), "pyref_lizard.lizard_encode", inputs={"data": data}, enqueue_only=True)
        pts = enc + [b"\xff" * 32, pyref_h2c.ristretto_hash_from_bytes(b"no payload")]
        payload, status = [], []
        for e in pts:
            pt = pyref_lizard.ristretto_decode(e)
            got = None if pt is None else pyref_lizard.lizard_decode(pt)
            payload.append(bytes(16) if got is None else got)
            status.append(2 if pt is None else (0 if got is None else 1))
        add("hash.lizard_decode", lambda b, d: b.eng.ristretto_lizard_decode_batch_t(d["pts"]), (arr(payload, 16), np.array(status, np.uint8)),
            "pyref_lizard.ristretto_decode, pyref_lizard.lizard_decode", inputs={"pts": arr(pts)}, enqueue_only=True, statuses=status)

    # -- the secret paths ---------------------------------------------------------------------------------------------------------------
    def _secret(self):
        orc, add = self.orc, self.add
        n = 33
        seeds = util.rand_bytes(4170, n)
        add("secret.keygen", lambda b, d: b.eng.keygen_batch_t(d["seeds"]), arr([orc.ed25519_pubkey(bytes(s)) for s in seeds]), "orc.ed25519_pubkey",
            inputs={"seeds": seeds}, enqueue_only=True)
        rng = np.random.default_rng(4171)
        msgs = [bytes(rng.integers(0, 256, (7 * i) % 150, dtype=np.uint8)) for i in range(n)]
        blob = np.frombuffer(b"".join(msgs) + bytes(16), np.uint8).copy()
        off = offsets([len(m) for m in msgs])
        pk = arr([orc.ed25519_pubkey(bytes(s)) for s in seeds])
        add("secret.sign", lambda b, d: b.eng.sign_batch_t(d["seeds"], d["blob"], d["off"]), (pk, arr([orc.ed25519_sign(bytes(seeds[i]), msgs[i]) for i in range(n)], 64)),
            "orc.ed25519_pubkey, orc.ed25519_sign", inputs={"seeds": seeds, "blob": blob, "off": off})
        ph = arr([orc.sha512(m) for m in msgs], 64)
        signed = [orc.ed25519_sign_prehashed(bytes(seeds[i]), bytes(ph[i]), b"sequence") for i in range(n)]
        assert all(st == 0 for st, _ in signed)
        add("secret.sign_prehashed", lambda b, d: b.eng.sign_batch_prehashed_t(d["seeds"], d["ph"], b"sequence"), (pk, arr([s for _, s in signed], 64)),
            "orc.ed25519_sign_prehashed", inputs={"seeds": seeds, "ph": ph})
        n = 40
        msgs, off, sigs, pks, _ = self.batch(n, lo=700)
        sigs[5, 3] ^= 1
        sigs[17, 32:] = np.frombuffer(i2b(b2i(sigs[17, 32:]) + L), np.uint8)
        pks[29] = arr([BAD_POINT])[0]
        _, each = self.verdicts(msgs, off, sigs, pks)
        add("secret.verify_each", lambda b, d: b.eng.verify_each_t(d["msgs"], d["off"], d["sigs"], d["pks"]), np.array(each, np.uint8), "orc.ed25519_verify",
            inputs={"msgs": msgs, "off": off, "sigs": sigs, "pks": pks}, enqueue_only=True, defects={5: VERIFY, 17: SCALAR_FORMAT, 29: NONE})

    # -- the host-pointer forms ---------------------------------------------------------------------------------------------------------
    def _host(self):
        orc, add = self.orc, self.add
        mu_mb, mu_x = ffi_min_units()
        n_mb = smallest(lambda n: ffi_chunks(n, mu_mb) >= 2)
        n_x = smallest(lambda n: ffi_chunks(n, mu_x) >= 2)
        s = util.rand_scalars(4180, n_mb)
        add("host.mul_base", lambda b, d: b.eng.mul_base_batch(s), orc.mul_base_compress_batch(s, threads=THREADS), "orc.mul_base_compress_batch", n=n_mb, min_units=mu_mb)
        k, u = util.rand_bytes(4181, n_x), util.rand_bytes(4182, n_x)
        add("host.x25519", lambda b, d: b.eng.x25519_batch(k, u), orc.x25519_batch(k, u, threads=THREADS), "orc.x25519_batch", n=n_x, min_units=mu_x)
        n = 300
        add("host.msm", lambda b, d: b.eng.msm_vartime(self.x[:n], self.enc[:n], in_fmt=ED, out_fmt=ED), (OK, self.PB(sum(v * v for v in self.X[:n]))),
            "orc.ed_mul_base(sum x_i^2 mod l)", n=n)
        for variant, z in (("honest", Z_TRANSCRIPT), ("forged", Z_DEVICE)):
            msgs, off, sigs, pks, j = self.batch(64, variant, lo=900)
            want, each = self.verdicts(msgs, off, sigs, pks)
            M = [bytes(msgs[int(off[i]):int(off[i + 1])]) for i in range(64)]
            add("host.verify.%s.z%d" % (variant, z), lambda b, d, M=M, S=rows(sigs), K=rows(pks), z=z: b.eng.verify_batch(M, S, K, z), want, "orc.ed25519_verify_batch",
                n=64, variant=variant, defect=j, each=each, status=OK if variant == "honest" else VERIFY)


_CATALOGUE = None


def catalogue(orc):
    """the catalogue, built once per process"""
    global _CATALOGUE
    if _CATALOGUE is None:
        _CATALOGUE = Catalogue(orc)
    return _CATALOGUE
