"""Constant-time posture of the Lizard kernels, checked on the compiled code (hipcc -S for gfx950, no GPU needed).

The Lizard payload is data to be kept secret (an ElGamal plaintext), and the reference computes encode, decode and
map_to_curve_inverse with conditional selects only (lizard/lizard_ristretto.rs, lizard/jacobi_quartic.rs).  csrc/lizard.hip
k_lizard_encode, k_lizard_decode and k_map_to_curve_inverse are written the same way: the eight candidates are visited by a
uniform loop whose Jacobi point is picked by selects on the loop counter.  The compiler could still turn a select into a branch
on "does any lane want this", so the property is asserted on the instruction stream: in every instantiation (both point formats)
the only exec-mask operation is the bounds exit (one s_and_saveexec and one branch on exec), and there is no branch on vcc.
The loops left are uniform (scalar, SCC): the exponentiation chains, the SHA-256 rounds and the candidate loop.  There is no
scratch traffic (no register array indexed at run time) and no call.  Item i reads and writes its own slots only."""
import os
import re

import pytest

from util import HIPCC, asm_functions, asm_ops, device_asm

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


@pytest.fixture(scope="module")
def lizard_asm(tmp_path_factory):
    return device_asm(tmp_path_factory, "lizard")


def _functions(lines, pattern):
    """-> {mangled name: opcodes} of the matching functions"""
    return {name: asm_ops(body) for name, body in asm_functions(lines, pattern).items()}


@pytest.mark.parametrize("kernel,min_ops", [("k_lizard_encode", 2000), ("k_lizard_decode", 3000), ("k_map_to_curve_inverse", 3000)])
def test_lizard_kernels_have_no_data_branch(lizard_asm, kernel, min_ops):
    fns = _functions(lizard_asm, r"_ZN6c25519\d+" + kernel + r"ILi[01]E")
    assert len(fns) == 2, sorted(fns)
    for name, ops in fns.items():
        saveexec = [o for o in ops if "saveexec" in o]
        exec_br = [o for o in ops if o.startswith("s_cbranch_exec")]
        vcc_br = [o for o in ops if o.startswith("s_cbranch_vcc")]
        assert len(saveexec) == 1 and len(exec_br) == 1, (name, saveexec, exec_br)      # the bounds exit
        assert not vcc_br, (name, vcc_br)
        assert not any(o.startswith(("s_swappc", "scratch_", "buffer_")) for o in ops), name      # no calls, no scratch traffic
        assert len(ops) > min_ops, (name, len(ops))


def test_lizard_kernels_use_no_scratch(lizard_asm):
    text = "\n".join(lizard_asm)
    sizes = re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)
    names = re.findall(r"\.name:\s+(_ZN6c25519\S*k_(?:lizard|map_to_curve_inverse)\S*)", text)
    assert len(names) == 6, names
    assert sizes and all(int(s) == 0 for s in sizes), sizes
