"""Constant-time posture of the hash-to-group MAP kernels, checked on the compiled code (hipcc -S for gfx950, no GPU needed).

RistrettoPoint::from_uniform_bytes / map_to_curve take inputs that may be secrets (an OPAQUE / OPRF client's password hash), and
the reference computes them with conditional selects only (ristretto/elligator.rs:15-52).  csrc/h2c.hip k_ristretto_from_uniform and
k_ristretto_map are written the same way; the compiler could still turn a select into a branch on "does any lane want this", so
the property is asserted on the instruction stream: in every instantiation (both output formats) the only exec-mask operation is
the bounds exit (one s_and_saveexec and one branch on exec), and there is no branch on vcc.  The loops left are the uniform
(scalar, SCC) loops of the exponentiation chains.  No data-dependent memory address exists in these kernels: item i reads and
writes its own slots only."""
import os

import pytest

from util import HIPCC, asm_functions, asm_ops, device_asm

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")


@pytest.fixture(scope="module")
def h2c_asm(tmp_path_factory):
    return device_asm(tmp_path_factory, "h2c")


def _functions(lines, pattern):
    """-> {mangled name: opcodes} of the matching functions"""
    return {name: asm_ops(body) for name, body in asm_functions(lines, pattern).items()}


@pytest.mark.parametrize("kernel", ["k_ristretto_from_uniform", "k_ristretto_map"])
def test_map_kernels_have_no_data_branch(h2c_asm, kernel):
    fns = _functions(h2c_asm, r"_ZN6c25519\d+" + kernel + r"ILi[01]E")
    assert len(fns) == 2, sorted(fns)
    for name, ops in fns.items():
        saveexec = [o for o in ops if "saveexec" in o]
        exec_br = [o for o in ops if o.startswith("s_cbranch_exec")]
        vcc_br = [o for o in ops if o.startswith("s_cbranch_vcc")]
        assert len(saveexec) == 1 and len(exec_br) == 1, (name, saveexec, exec_br)      # the bounds exit
        assert not vcc_br, (name, vcc_br)
        assert not any(o.startswith(("s_swappc", "scratch_", "buffer_")) for o in ops), name      # no calls, no scratch traffic
        assert len(ops) > 3000, (name, len(ops))          # (the maps really are in there)
