"""Constant-time posture of the group-law kernels, checked on the compiled code (hipcc -S for gfx950, no GPU needed).

csrc/group.hip adds, subtracts, negates, multiplies by the cofactor and compares points one item per lane with selects only, and sums
segments with a per-lane fold and a shuffle scan whose every choice is a select too.  The compiler could still turn a select into a branch
on "does any lane want this", so the property is asserted on the instruction stream:
- elementwise and equality kernels: the only exec-mask operation is the bounds exit (one s_and_saveexec and one branch on exec);
- the segmented sum: its exec branches guard the stores of finished sums and pieces, whose conditions come from the segment keys (the
  public offsets); it has no branch on vcc (per-lane data: every loop is counted in SGPRs), and its count of exec branches is fixed;
- no kernel has scratch traffic or a call."""
import os
import re

import pytest

from util import HIPCC, asm_functions, asm_ops as _ops, device_asm

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
# kernel, instantiations, minimum instruction count of each
ELEMENTWISE = [("k_group_elem", 22, 200), ("k_group_eq", 8, 300)]


@pytest.fixture(scope="module")
def group_asm(tmp_path_factory):
    return device_asm(tmp_path_factory, "group")


def _functions(lines, kernel):
    """{mangled name: [lines of the body]} of the kernel's instantiations"""
    return asm_functions(lines, r"_ZN6c25519\d+" + kernel + r"(?:E|I)")


def _branches(ops):
    saveexec = [o for o in ops if "saveexec" in o]
    exec_br = [o for o in ops if o.startswith("s_cbranch_exec")]
    vcc_br = [o for o in ops if o.startswith("s_cbranch_vcc")]
    other_br = [o for o in ops if o.startswith("s_cbranch") and not o.startswith(("s_cbranch_exec", "s_cbranch_scc"))]
    return saveexec, exec_br, vcc_br, other_br


@pytest.mark.parametrize("kernel,count,min_ops", ELEMENTWISE)
def test_elementwise_kernels_have_no_data_branch(group_asm, kernel, count, min_ops):
    fns = _functions(group_asm, kernel)
    assert len(fns) == count, sorted(fns)
    for name, body in fns.items():
        ops = _ops(body)
        saveexec, exec_br, vcc_br, other_br = _branches(ops)
        assert len(saveexec) == 1 and len(exec_br) == 1, (name, saveexec, exec_br)      # the bounds exit
        assert not vcc_br and not other_br, (name, vcc_br, other_br)
        assert not any(o.startswith(("s_swappc", "s_setpc", "scratch_", "buffer_")) for o in ops), name
        assert len(ops) > min_ops, (name, len(ops))


def test_segmented_sum_branches_on_keys_only(group_asm):
    fns = _functions(group_asm, "k_seg_sum")
    assert len(fns) == 4, sorted(fns)                          # levels 0 (Edwards, Ristretto, RAW160 input) and the piece levels
    for name, body in fns.items():
        ops = _ops(body)
        saveexec, exec_br, vcc_br, other_br = _branches(ops)
        assert not vcc_br and not other_br, (name, vcc_br, other_br)
        # the bounds exit, the in-loop store of a sum complete in its lane, the closing lane's head piece / final sum, and lane 63's pieces
        assert 4 <= len(saveexec) <= 10 and 4 <= len(exec_br) <= 12, (name, saveexec, exec_br)
        assert not any(o.startswith(("s_swappc", "s_setpc", "scratch_", "buffer_")) for o in ops), name
        # the point arithmetic is there: at least K + 7 additions' worth of 32 x 32 -> 64 multiplies
        assert sum(o == "v_mad_u64_u32" for o in ops) > 700, name


def test_group_kernels_use_no_scratch(group_asm):
    text = "\n".join(group_asm)
    names = re.findall(r"\.name:\s+(_ZN6c25519\S*k_(?:group|seg)_\S*)", text)
    assert len(names) == 22 + 8 + 4 + 2 + 2, names            # elementwise, eq, sum levels, finish, keys + any_bad
    sizes = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)
    assert sizes and all(int(s) == 0 for s in sizes), sizes
