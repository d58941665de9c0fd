"""The workspace layouts of csrc, on the host (no GPU): ws_layout (csrc/capi_util.h), the one helper every entry point carves its device
workspace with, and the two sized structs built on it, straus_ws (csrc/straus.h) and segb_ws (csrc/mid_segb.h).

tests/host/ws_layout_host.cpp is a program with a main of its own (nothing is loaded into python), compiled for the host alone with the
address and undefined-behaviour sanitizers; its ctx_reserve hands out a host buffer of exactly the bytes asked for, and the program writes
every byte of every part, so a part that leaves the reservation ends the run.

tests/golden/ws_layout_totals.json holds the totals of straus_ws and segb_ws as the hand-summed structs gave them before they were built on
ws_layout (m in {0, 1, 3}, maxt in {1, 64, 2049}, both output formats, with and without a caller's ok array): a call must go on reserving
exactly those bytes."""
import json
import os
import subprocess

import pytest

import util

ROOT = util.ROOT
pytestmark = pytest.mark.skipif(not os.path.exists(util.HIPCC), reason="hipcc not available")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ws_layout") / "ws_layout_host")
    subprocess.check_call([util.HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-w",
                           os.path.join(ROOT, "tests", "host", "ws_layout_host.cpp"), "-o", out])
    return out


def _run(exe, *args):
    env = dict(os.environ); env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=1"; env["UBSAN_OPTIONS"] = "halt_on_error=1"
    r = subprocess.run([exe] + [str(a) for a in args], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    return r.stdout


def _al256(b):
    return (b + 255) // 256 * 256


@pytest.mark.parametrize("slack", [0, 16, 256])
@pytest.mark.parametrize("sizes", [[1], [0], [256, 0, 0, 257], [0, 1, 255, 256, 257, 0, 1000, 160 * 2049], [64 * 5, 16 * 9, 32 * 11, 0, 40], []])
def test_parts_are_aligned_disjoint_and_in_order(exe, sizes, slack):
    rows = [[int(x) for x in line.split()] for line in _run(exe, "parts", slack, *sizes).splitlines()]
    parts, (total, with_slack, reserved) = rows[:-1], rows[-1]
    assert len(parts) == len(sizes)
    at = 0
    for (off, ptr_off), b in zip(parts, sizes):
        assert off == at and ptr_off == off and off % 256 == 0           # in declaration order, each where the last one ended: disjoint
        at += _al256(b)                                                  # (a part of 0 bytes consumes nothing: the next one has its offset)
        assert at - off >= b
    assert total == at == sum(_al256(b) for b in sizes)
    assert with_slack == reserved == total + slack                       # bytes(slack) is the sum of the parts plus the slack, and what reserve() asks for


def test_sized_structs_reserve_what_they_always_did(exe):
    got = json.loads(_run(exe, "totals"))
    with open(os.path.join(ROOT, "tests", "golden", "ws_layout_totals.json")) as fh:
        want = json.load(fh)
    assert len(want["straus_ws"]) == 3 * 3 * 2 * 2 and len(want["segb_ws"]) == 3 * 3
    assert got == want
