"""Constant-time posture of the Montgomery kernels, checked on the compiled code (hipcc -S for gfx950, no GPU needed).

csrc/montgomery.hip runs the ladder of montgomery.rs:183-211 on secret scalars and bit strings, and to_edwards on points, one item per
lane with selects only.  The compiler could still turn a select into a branch on "does any lane want this", so the property is asserted
on the instruction stream of every kernel: the only exec-mask operation is the bounds exit (one s_and_saveexec and one branch on exec),
there is no branch on vcc (which would follow per-lane data), every other branch is on SCC (scalar, uniform), and there is no scratch
traffic and no call.  The mul_bits_be loop must be counted in SGPRs: its trip count is the kernel argument nbits, never lane data."""
import os
import re

import pytest

from util import HIPCC, asm_functions, asm_ops as _ops, device_asm

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
KERNELS = [("k_mont_mul", 1, 1200), ("k_mont_mul_bits", 1, 1200), ("k_mont_to_edwards_prep", 1, 40), ("k_mont_to_edwards", 4, 5000)]


@pytest.fixture(scope="module")
def mont_asm(tmp_path_factory):
    return device_asm(tmp_path_factory, "montgomery")


def _functions(lines, kernel):
    """{mangled name: [lines of the body]} of the kernel's instantiations"""
    return asm_functions(lines, r"_ZN6c25519\d+" + kernel + r"(?:E|I)")


@pytest.mark.parametrize("kernel,count,min_ops", KERNELS)
def test_montgomery_kernels_have_no_data_branch(mont_asm, kernel, count, min_ops):
    fns = _functions(mont_asm, kernel)
    assert len(fns) == count, sorted(fns)
    for name, body in fns.items():
        ops = _ops(body)
        saveexec = [o for o in ops if "saveexec" in o]
        exec_br = [o for o in ops if o.startswith("s_cbranch_exec")]
        vcc_br = [o for o in ops if o.startswith("s_cbranch_vcc")]
        other_br = [o for o in ops if o.startswith("s_cbranch") and not o.startswith(("s_cbranch_exec", "s_cbranch_scc"))]
        assert len(saveexec) == 1 and len(exec_br) == 1, (name, saveexec, exec_br)      # the bounds exit
        assert not vcc_br and not other_br, (name, vcc_br, other_br)
        assert not any(o.startswith(("s_swappc", "s_setpc", "scratch_", "buffer_")) for o in ops), name      # no calls, no scratch traffic
        assert len(ops) > min_ops, (name, len(ops))


def test_mul_bits_loop_is_counted_in_sgprs(mont_asm):
    (body,) = _functions(mont_asm, "k_mont_mul_bits").values()
    heads = [i for i, l in enumerate(body) if "Loop Header" in l]
    assert len(heads) == 1, heads                              # one loop: the ladder steps (the word fetch is inside it)
    label = body[heads[0]].split(":")[0]
    back = [i for i, l in enumerate(body) if i > heads[0] and re.match(r"^\s+s_cbranch_scc[01]\s+" + re.escape(label) + r"\b", l)]
    assert len(back) == 1, (label, back)                       # the back edge is a branch on SCC ...
    cmp = [l.split() for l in body[heads[0]:back[0]] if re.match(r"^\s+s_cmp", l)]
    assert cmp and all(not any(t.startswith("v") for t in c[1:]) for c in cmp), cmp    # ... set by a scalar compare of SGPRs
    # the bits are fetched with byte loads (one 32-bit word per 32 steps, at an offset from the loop counter) in a block of the loop:
    # the compiler may rotate it in front of the header, entered from the latch by a jump
    targets = {l.split()[1] for l in body[heads[0]:back[0] + 3] if re.match(r"^\s+s_(c?branch)\S*\s+\.LBB", l)}
    in_loop, cur = [], None
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\S+):", l)
        if m:
            cur = m.group(1)
        if re.match(r"^\s+global_load", l):
            in_loop.append((l.split()[0], heads[0] <= i <= back[0] or cur in targets and cur != label))
    loads = [o for o, inside in in_loop if inside]
    assert loads == ["global_load_ubyte"] * 4, in_loop


def test_montgomery_kernels_use_no_scratch(mont_asm):
    text = "\n".join(mont_asm)
    sizes = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)
    names = re.findall(r"\.name:\s+(_ZN6c25519\S*k_mont\S*)", text)
    assert len(names) == 7, names
    assert sizes and all(int(s) == 0 for s in sizes), sizes
