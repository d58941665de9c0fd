"""The catalogue of tests/call_catalogue.py, checked without a GPU: every step carries an expectation made by the references, the shapes reach
every route the sequence tests (tests/test_gpu_call_sequences.py) are meant to mix -- asked of the library's own host-arithmetic planners, so a
boundary that moves fails HERE instead of the GPU tests silently losing a route -- and every failing variant fails for the reason, at the
place and with the status the references give."""
import fnmatch
import re

import numpy as np
import pytest

import call_catalogue as C

L = C.L


@pytest.fixture(scope="module")
def cat(orc):
    return C.catalogue(orc)


@pytest.fixture(scope="module")
def E():
    import curve25519_dalek_amd as pkg
    return pkg.Engine


def steps(cat, pattern):
    out = [s for s in cat.steps if fnmatch.fnmatchcase(s.name, pattern)]
    assert out, pattern
    return out


def test_every_step_has_a_reference_expectation(cat):
    assert len(cat.steps) >= 80 and {s.family for s in cat.steps} == set(C.FAMILIES)
    for s in cat.steps:
        assert s.want is not None and callable(s.fn), s.name
        assert re.search(r"orc\.|pyref_|mod l|invariant|c25519_hip\.h", s.ref), (s.name, s.ref)
        if isinstance(s.want, C.Raises):
            assert s.want.part and s.norm is None, s.name
        for k, a in s.inputs.items():                       # device inputs: what Engine._t asks of a tensor
            assert isinstance(a, np.ndarray) and a.flags["C_CONTIGUOUS"] and a.dtype in (np.uint8, np.int64), (s.name, k)


def test_enqueue_only_table_covers_every_step(cat):
    """the table of the module docstring: every step falls under exactly one row, and is flagged as that row says"""
    table = re.findall(r"^  (\S(?:.*?\S)?)\s{2,}(\S(?:.*?\S)?)\s{2,}(\S.*)$", C.__doc__, re.M)
    table = [(pats.split(", "), visit) for pats, _, visit in table if not pats.startswith(("step (", "---"))]
    assert len(table) >= 25
    for s in cat.steps:
        hits = [visit for pats, visit in table if any(fnmatch.fnmatchcase(s.name, p) for p in pats)]
        assert len(hits) == 1, (s.name, hits)
        assert hits[0].startswith("enqueue only") == s.enqueue_only, (s.name, hits[0])
    assert len(cat.enqueue_only()) >= 20


def test_msm_and_verify_paths(cat, E):
    """small, mid and pipeline for both kinds, each at the smallest n of its path"""
    for kind, found in ((0, cat.msm_n), (1, cat.verify_n)):
        for path, n in found.items():
            assert E.msm_route(kind, n, C.ED)["path"] == path
            assert n == 1 or E.msm_route(kind, n - 1, C.ED)["path"] != path
    for suffix in ("ok", "none", "bit255"):
        got = {}
        for s in steps(cat, "msm.*." + suffix):
            assert s.inputs["x"].shape[0] == s.inputs["enc"].shape[0] == s.meta["n"]
            got.setdefault(E.msm_route(0, s.meta["n"], C.ED)["path"], []).append(s.meta["n"])
            assert E.msm_route(0, s.meta["n"], C.ED)["path"] == s.meta["route"]
        assert set(got) == {"small", "mid", "pipeline"} and all(min(got[p]) == cat.msm_n[p] for p in got), (suffix, got)
    assert {E.msm_route(0, s.meta["n"], C.ED)["path"] for s in steps(cat, "msm.partial_record.*")} == {"small", "mid"}
    for variant in ("honest", "forged", "noncanonical", "badkey"):
        for z in (0, 1):
            got = {E.msm_route(1, s.meta["n"])["path"]: s.meta["n"] for s in steps(cat, "verify.*.%s.z%d" % (variant, z))}
            assert {"small", "mid"} <= set(got) and got["mid"] == cat.verify_n["mid"], (variant, z, got)
            assert {s.meta["n"] for s in steps(cat, "verify.*.%s.z%d" % (variant, z))} >= {1, 64}
    big = cat.by_name["verify.pipeline.honest.z1"]
    assert E.msm_route(1, big.meta["n"])["path"] == "pipeline" and big.meta["n"] == cat.verify_n["pipeline"] == big.inputs["sigs"].shape[0]
    for s in steps(cat, "verify.*"):
        assert E.msm_route(1, s.meta["n"])["path"] == s.meta["route"] and s.inputs["sigs"].shape[0] == s.meta["n"], s.name


def test_segment_routes(cat, E):
    import curve25519_dalek_amd.engine as eng
    for s in steps(cat, "seg.msm.*"):
        routes = set(E.msm_vartime_segments_routes(s.meta["seg_off"]).tolist())
        assert routes == {eng.MSM_SEGMENT_ROUTE_LANE, eng.MSM_SEGMENT_ROUTE_WAVE, eng.MSM_SEGMENT_ROUTE_BUCKET}, routes
        assert int(s.meta["seg_off"][-1]) == s.inputs["s"].shape[0] == s.inputs["enc"].shape[0]
        assert 0 in np.diff(s.meta["seg_off"])                                             # an empty segment
    for s in steps(cat, "seg.verify.*"):
        off = s.meta["seg_off"]
        assert sorted(np.diff(off).tolist()) == [0, 1, 17, 300]
        segmented, single, passes, _ = E.verify_batch_segments_plan(off)
        assert (segmented, single) == (len(off) - 1, 0) and passes >= 1
        on_device, on_host = E.batch_transcript_zs_segments_plan(off)
        assert on_device >= 1 and on_host >= 1, "both the device and the host transcript"
        lane_or_wave = set(E.msm_vartime_segments_routes(np.concatenate([[0], np.cumsum(2 * np.diff(off) + 1)])).tolist())
        assert lane_or_wave == {eng.MSM_SEGMENT_ROUTE_LANE, eng.MSM_SEGMENT_ROUTE_WAVE}     # 2k + 1 terms per segment (include/c25519_hip.h)


def test_precomp_routes(cat, E):
    import curve25519_dalek_amd.engine as eng
    lane, wave = cat.by_name["precomp.rows_lane"], cat.by_name["precomp.rows_wave"]
    assert E.precomp_msm_vartime_rows_plan(lane.meta["m"], lane.meta["w"])[0] == eng.PRECOMP_ROWS_LANE
    assert E.precomp_msm_vartime_rows_plan(lane.meta["m"] - 1, lane.meta["w"])[0] == eng.PRECOMP_ROWS_WAVE      # the smallest such m
    assert E.precomp_msm_vartime_rows_plan(wave.meta["m"], wave.meta["w"])[0] == eng.PRECOMP_ROWS_WAVE
    for s in (lane, wave):
        assert s.inputs["sc"].shape == (s.meta["m"], s.meta["w"], 32) and s.meta["w"] <= len(cat.static_k)
    assert 8 <= len(cat.static_k) <= 16
    for name in ("precomp.mixed_rows", "precomp.fold"):
        s = cat.by_name[name]
        route, _, passes, most = E.precomp_msm_vartime_mixed_rows_plan(s.meta["m"], s.meta["w"], s.meta["dyn_off"])
        assert route in (eng.PRECOMP_ROWS_LANE, eng.PRECOMP_ROWS_WAVE) and passes == 1 and most == int(s.meta["dyn_off"][-1]) == s.inputs["ds"].shape[0]
    s = cat.by_name["precomp.fold"]
    assert E.precomp_msm_vartime_mixed_rows_fold_plan(s.meta["m"], s.meta["w"], s.meta["dyn_off"], 16)[:2] == (s.meta["w"], s.inputs["ds"].shape[0])


def test_host_forms_are_cut_into_chunks(cat):
    """mul_base_batch and x25519_batch at the smallest n that ffi_chunk_units (csrc/ffi.h) cuts into two chunks, with the min_units of their callers"""
    assert C.ffi_chunk_units(0, 1 << 16) == 1 and C.ffi_chunk_units(5, 1 << 16) == 5 and C.ffi_chunk_units((1 << 17) + 1, 1 << 16) == (1 << 16) + 1024
    assert C.ffi_chunk_units(1 << 30, 1 << 16) == (1 << 30) // C.ffi_maxch()
    src = open(C.os.path.join(C.CSRC, "ffi.h")).read()
    for line in ("if (n <= min_units) return n ? n : 1;", "uint64_t nch = n / min_units;", "if (nch > (uint64_t)c25519_ctx::FFI_MAXCH) nch = c25519_ctx::FFI_MAXCH;",
                 "const uint64_t c = (n + nch - 1) / nch;", "return (c + 1023) & ~(uint64_t)1023;"):
        assert line in src, "csrc/ffi.h ffi_chunk_units changed: restate it in tests/call_catalogue.py (%s)" % line
    mins = dict(zip(("host.mul_base", "host.x25519"), C.ffi_min_units()))
    for name, mu in mins.items():
        s = cat.by_name[name]
        assert s.meta["min_units"] == mu and C.ffi_chunks(s.meta["n"], mu) >= 2 and C.ffi_chunks(s.meta["n"] - 1, mu) == 1, name
        assert s.want.shape == (s.meta["n"], 32)


def test_failing_variants_fail_where_the_references_say(cat, orc):
    assert orc.ed_decompress(C.BAD_POINT) is None
    bad = np.frombuffer(C.BAD_POINT, np.uint8)
    seen = 0
    for s in cat.steps:
        if "bad_rows" in s.meta:                             # exactly these rows hold the point that does not decode
            enc = s.inputs.get("enc", s.inputs.get("q"))
            hit = np.nonzero((enc == bad).all(axis=1))[0].tolist()
            assert hit == s.meta["bad_rows"] and orc.ed_decompress_ok_batch(enc, threads=C.THREADS).tolist() == [0 if i in hit else 1 for i in range(enc.shape[0])], s.name
            seen += 1
    assert seen >= 8
    for s in steps(cat, "msm.*.bit255"):
        assert int((s.inputs["x"][:, 31] >> 7).sum()) == 1 and isinstance(s.want, C.Raises)
    for s in steps(cat, "msm.*.none"):
        assert s.want == (C.NONE,) and s.meta["status"] == C.NONE
    for s in steps(cat, "*bad_off*"):
        assert (np.diff(s.inputs["off"]) < 0).any() and isinstance(s.want, C.Raises)


def test_verify_variants_have_the_oracles_verdicts(cat, orc):
    """the oracle accepts the honest batches, rejects exactly the defective signature of the others, with the status the batch call must give"""
    code = {"honest": C.OK, "forged": C.VERIFY, "noncanonical": C.SCALAR_FORMAT, "badkey": C.NONE}
    checked = 0
    for s in cat.steps:
        if "variant" not in s.meta or "each" not in s.meta:
            continue
        v, each, j = s.meta["variant"], s.meta["each"], s.meta["defect"]
        want = s.want[1] if s.family == "chain" else s.want
        assert want == code[v] == s.meta["status"], s.name
        assert [i for i, st in enumerate(each) if st != 0] == ([] if v == "honest" else [j]), s.name
        assert v == "honest" or each[j] == code[v], s.name
        if "sigs" in s.inputs:
            canonical = [orc.sc_is_canonical(bytes(r[32:])) for r in s.inputs["sigs"]]
            assert [i for i, c in enumerate(canonical) if not c] == ([j] if v == "noncanonical" else []), s.name
        checked += 1
    assert checked >= 30
    assert cat.by_name["verify.pipeline.honest.z1"].want == C.OK
    for s in steps(cat, "seg.verify.*"):
        p = s.meta["poisoned"]
        assert s.want.tolist() == [C.VERIFY if k == p else C.OK for k in range(len(s.want))]
        assert [k for k, e in enumerate(s.meta["each"]) if any(e)] == [p] and sum(1 for st in s.meta["each"][p] if st) == 1
    s = cat.by_name["seg.msm.none"]
    assert s.want[0] == C.NONE and s.want[2].tolist() == [0 if k == s.meta["poisoned"] else 1 for k in range(len(s.want[2]))]
    assert E_routes_of_poisoned(s) == 1                      # the poisoned segment is a wave segment
    s = cat.by_name["secret.verify_each"]
    assert {i: int(st) for i, st in enumerate(s.want) if st} == s.meta["defects"]
    s = cat.by_name["hash.lizard_decode"]
    assert set(s.meta["statuses"]) == {0, 1, 2}, "a payload, no payload and a bad encoding"


def E_routes_of_poisoned(s):
    import curve25519_dalek_amd as pkg
    return int(pkg.Engine.msm_vartime_segments_routes(s.meta["seg_off"])[s.meta["poisoned"]])
