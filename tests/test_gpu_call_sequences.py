"""Calls in SEQUENCE on one context, on side streams and across stream rebinding (the steps and their references: tests/call_catalogue.py).

One c25519_ctx shares its workspaces (scratch, prefix, tmp_a .. tmp_f, dom, pts_all), the 256-byte flag block, the result slots, the page-locked
publication slot with its sequence number, a peer context, the aux and copy streams and a handful of events between ALL entry points
(csrc/ctx.h); consecutive calls are kept apart by stream order, those events, per-call zeroing and the ev_rebind hand-over of
c25519_ctx_set_stream alone.  Every other GPU test makes one kind of call at a time on torch's default stream and reads the result before the
next call; here every step of the catalogue follows every other one on one context, enqueue-only calls are queued without a host visit in
between, the context is bound to non-default torch streams, rebound between streams from call to call (the first execution of the ev_rebind
branch), and left on the non-blocking stream c25519_ctx_create gives it (the Rust shim's configuration).  Failing calls are steps like the
others, so "a failed call leaves no trace" and "a passing call does not lend its OK word to a failing one" are covered in both orders.

Not covered: the branch of c25519_ctx_set_stream for an old stream the caller has destroyed (torch never destroys its pooled streams), two
host threads on one context (the contract forbids overlapping calls), several GPUs or processes."""
import os
import re
import time

import numpy as np
import pytest

import call_catalogue as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import curve25519_dalek_amd as p
    return p


@pytest.fixture(scope="module")
def cat(orc):
    return C.catalogue(orc)


class _Fresh:
    """a fresh Engine bound to the catalogue, closed on exit"""

    def __init__(self, pkg, cat, cls=None):
        self.b = C.Bound((cls or pkg.Engine)(0), cat)

    def __enter__(self):
        return self.b

    def __exit__(self, *exc):
        self.b.close()
        self.b.eng.close()


def _ready(b, steps):
    """inputs on the device and handles built, everything drained: nothing below waits for an upload"""
    import torch
    b.prepare(steps)
    torch.cuda.synchronize()


def _check_all(done, what):
    bad = [e for e in (C.check(s, raw) for s, raw in done) if e]
    assert not bad, "%s: %d of %d calls differ from their references\n%s" % (what, len(bad), len(done), "\n".join(bad[:6]))


def _clock(name, t0, extra=""):
    print("%s: %.2f s%s" % (name, time.perf_counter() - t0, extra))


# ---- 1. every step alone: a failure below is then the sequence's ------------------------------------------------------------------
@pytest.mark.parametrize("family", C.FAMILIES)
def test_each_step_alone(pkg, cat, family):
    t0 = time.perf_counter()
    for s in cat.family(family):
        with _Fresh(pkg, cat) as b:
            err = C.check(s, b.run(s))
        assert not err, err
    _clock("test_each_step_alone[%s]" % family, t0, ", %d steps" % len(cat.family(family)))


# ---- 2. every ordered pair on ONE engine --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one(pkg, cat):
    b = C.Bound(pkg.Engine(0), cat)
    b.history = []
    b.pairs = 0
    yield b
    b.close()
    b.eng.close()


@pytest.mark.parametrize("family", C.FAMILIES)
def test_every_ordered_pair(one, cat, family):
    """A then B for every A of the family and every B of the catalogue, with no look at A's device outputs in between (an enqueue-only A has
    not been waited for when B starts); both must equal their references.  One engine serves all ten cases, so the pairs follow each other too."""
    t0 = time.perf_counter()
    _ready(one, cat.steps)
    for A in cat.family(family):
        for B in cat.steps:
            ra = one.run(A)
            rb = one.run(B)
            ea, eb = C.check(A, ra), C.check(B, rb)
            assert not (ea or eb), "pair (%s, %s) after %s:\n%s" % (A.name, B.name, one.history[-3:], "\n".join(e for e in (ea, eb) if e))
            one.history += [A.name, B.name]
            one.pairs += 1
    _clock("test_every_ordered_pair[%s]" % family, t0, ", %d pairs (%d so far)" % (len(cat.family(family)) * len(cat.steps), one.pairs))


# ---- 3. enqueue-only calls queued behind each other, one host visit at the end ------------------------------------------------------
def test_enqueue_only_queue(pkg, cat, orc):
    import torch
    t0 = time.perf_counter()
    steps = cat.enqueue_only()
    big = C.util.rand_scalars(4190, 1 << 16)
    want_big = orc.mul_base_compress_batch(big, threads=C.THREADS)
    with _Fresh(pkg, cat) as b:
        _ready(b, steps)
        dbig = torch.from_numpy(big).cuda()
        out_big = torch.empty((1 << 16, 32), dtype=torch.uint8, device="cuda")
        for attempt in ("warm-up", "queued"):               # the first time round grows the workspaces and fills torch's allocator: the second allocates nothing
            torch.cuda.synchronize()
            b.eng.mul_base_batch_t(dbig, out=out_big)       # a few milliseconds of work in front of the queue
            done = [(s, b.run(s)) for _ in range(3) for s in steps]
            torch.cuda.synchronize()
            assert np.array_equal(out_big.cpu().numpy(), want_big), attempt
            _check_all(done, "enqueue-only queue (%s)" % attempt)
            del done
    _clock("test_enqueue_only_queue", t0, ", %d enqueue-only steps x 3" % len(steps))


# ---- 4. the whole catalogue on a non-default torch stream ----------------------------------------------------------------------------
def test_side_stream(pkg, cat):
    import torch
    t0 = time.perf_counter()
    with _Fresh(pkg, cat) as b:
        _ready(b, cat.steps)
        s = torch.cuda.Stream()
        assert s.cuda_stream != torch.cuda.current_stream().cuda_stream
        done = []
        with torch.cuda.stream(s):
            for step in cat.steps:
                d = {k: v.clone() for k, v in b.dev(step).items()}      # made on s just before the call: only stream order stands between the copy and the kernels
                done.append((step, b.run(step, d)))
                del d
        s.synchronize()
        _check_all(done, "side stream")
    _clock("test_side_stream", t0)


# ---- 5. rebinding between streams from call to call ------------------------------------------------------------------------------------
def test_rebinding_between_streams(pkg, cat):
    """Two walks through the catalogue, every call on another stream than the one before (s1, s2, default in turn; the step count is no multiple of 3, so the
    second walk pairs every step with other streams than the first).  B shares A's workspaces, so c25519_ctx_set_stream must make B's stream wait for A's."""
    import torch
    t0 = time.perf_counter()
    with _Fresh(pkg, cat) as b:
        _ready(b, cat.steps)
        streams = [torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.default_stream()]
        assert len({s.cuda_stream for s in streams}) == 3 and len(cat.steps) % 3, "the second walk must meet other streams than the first"
        done = []
        for i, step in enumerate(cat.steps + cat.steps):
            with torch.cuda.stream(streams[i % 3]):
                done.append((step, b.run(step)))
        torch.cuda.synchronize()
        _check_all(done, "rebinding")
    _clock("test_rebinding_between_streams", t0)


# ---- 6. the context's own non-blocking stream -----------------------------------------------------------------------------------------
def test_own_stream(pkg, cat):
    import torch

    class OwnStream(pkg.Engine):
        def _bind_stream(self):                              # never rebinds: the context keeps the stream c25519_ctx_create made
            if not self.ctx:
                raise pkg.EngineError("this Engine has been closed")

    t0 = time.perf_counter()
    with _Fresh(pkg, cat, OwnStream) as b:
        _ready(b, cat.steps)
        for step in cat.steps:
            torch.cuda.synchronize()                         # torch's streams know nothing of the context's: the inputs are ready, the last outputs read
            raw = b.run(step)
            b.eng.synchronize()
            err = C.check(step, raw)
            assert not err, err
        torch.cuda.synchronize()
        done = [(s, b.run(s)) for s in cat.family("chain") * 2]      # hram -> transcript -> record, twice each, nothing waited for in between
        b.eng.synchronize()
        _check_all(done, "own stream, chain")
    _clock("test_own_stream", t0)


# ---- 7. grow, shrink, trim ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("small,large", [("msm.small.ok", "msm.pipeline.ok"), ("verify.1.honest.z1", "verify.pipeline.honest.z1")])
def test_grow_shrink_trim(pkg, cat, small, large):
    t0 = time.perf_counter()
    small, large = cat.by_name[small], cat.by_name[large]
    with _Fresh(pkg, cat) as b:
        for what in (small, large, "trim", small, large, small):
            if what == "trim":
                b.eng.trim()
                ws = b.eng.workspaces()
                grown = {k: len(v) for k, v in ws.items() if k.split(".")[-1] not in ("d_flag", "d_slots") and len(v)}     # (the two fixed allocations: csrc/ctx.h)
                assert not grown and "scratch" in ws, grown
                continue
            err = C.check(what, b.run(what))
            assert not err, err
    _clock("test_grow_shrink_trim[%s]" % large.name, t0)


# ---- 8. more publications than there are slots ------------------------------------------------------------------------------------------
def test_many_publications(pkg, cat):
    import torch
    t0 = time.perf_counter()
    slots = int(re.search(r"C25519_MAX_SLOTS = (\d+)", open(os.path.join(C.CSRC, "ctx.h")).read()).group(1))
    rounds = 40
    assert rounds > 2 * slots
    msms = []
    for lo, n in ((0, 1), (1, 2), (3, 17), (20, 100), (10, 150)):                       # small path, RAW160 points: the route that publishes its record itself
        route = pkg.Engine.msm_route(0, n, C.RAW)
        assert route["path"] == "small" and route["publish"], route
        msms.append((torch.from_numpy(cat.x[lo:lo + n].copy()).cuda(), torch.from_numpy(cat.raw[lo:lo + n].copy()).cuda(), cat.PB(sum(v * v for v in cat.X[lo:lo + n]))))
    verifies = [cat.by_name[k] for k in ("verify.1.honest.z1", "verify.64.honest.z0", "verify.64.forged.z1", "verify.64.noncanonical.z0", "verify.1.badkey.z1")]
    hosts = [cat.by_name[k] for k in ("host.verify.honest.z0", "host.verify.forged.z1", "host.msm")]
    with _Fresh(pkg, cat) as b:
        _ready(b, verifies)
        lost, direct = b.eng.counter(1), b.eng.counter(2)
        for i in range(rounds):
            x, pts, want = msms[i % 5]
            assert b.eng.msm_vartime_t(x, pts, in_fmt=C.RAW, out_fmt=C.ED) == (C.OK, want), ("msm", i)
            for s in (verifies[i % 5], hosts[i % 3]):
                err = C.check(s, b.run(s))
                assert not err, (i, err)
        assert b.eng.counter(1) == lost, "a publication was lost and the call re-run"
        _clock("test_many_publications", t0, ", %d directly published calls of %d" % (b.eng.counter(2) - direct, 3 * rounds))
