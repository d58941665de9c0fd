"""Shared helpers for the GPU parity tests: seeded input generators (numpy) and oracle batch calls."""
import os
import re
import shutil
import subprocess

import numpy as np

L = 2**252 + 27742317777372353535851937790883648493
P = 2**255 - 19

# The release library reads no environment; the C25519_* knobs (A/B arms, pass-size overrides that make small inputs run many passes) exist only
# in the tuning build of the same sources (make tune, csrc/msm_internal.h C25519_KNOB).  Tests that need a knob run a fresh process on that file.
TUNE_LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "curve25519-dalek_amd", "lib", "libc25519hip_tune.so")


def tune_env(knobs=None, **more):
    """environment of a child process that loads the tuning build with the given C25519_* knobs set"""
    assert os.path.exists(TUNE_LIB), "run __graft_entry__.build() (make tune)"
    env = dict(os.environ, C25519_HIP_LIB=TUNE_LIB)
    env.update(knobs or {})
    env.update(more)
    return env


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child_argv(code):
    """argv of a child process that runs `code` against the library C25519_HIP_LIB of ITS environment names (the tuning / debug build).  The variable belongs to the
    TEST HARNESS: the package reads no environment (tests/test_abi_cpu.py asserts it); the child selects the build with an explicit select_library() call."""
    import sys
    pre = ("import os as _os, sys as _sys\n_sys.path.insert(0, %r)\n_p = _os.environ.get('C25519_HIP_LIB')\n"
           "if _p:\n    import curve25519_dalek_amd as _pkg\n    _pkg.select_library(_p)\n" % ROOT)
    return [sys.executable, "-c", pre + code]


def rand_bytes(seed, n, width=32):
    return np.random.default_rng(seed).integers(0, 256, size=(n, width), dtype=np.uint8)


def rand_scalars(seed, n):
    """uniform in [0, 2^252) -- canonical (reduced) scalars"""
    s = rand_bytes(seed, n)
    s[:, 31] &= 0x0F
    return s


def edge_scalars():
    vals = [0, 1, 2, 8, 31, 32, 33, 63, 64, 65, L - 1, L, L + 1, 2**252 - 1, 2**252, 2**255 - 1, 2**255 - 19,
            int.from_bytes(bytes([0xF8] + [0xFF] * 30 + [0x7F]), "little"), 2**254, 2**253 + 5, (1 << 255) - (1 << 200)]
    vals += [(1 << k) for k in range(0, 255, 17)] + [(1 << k) - 1 for k in range(5, 255, 23)]
    vals += [sum(32 << (6 * i) for i in range(42)), sum(31 << (6 * i) for i in range(42)), sum(63 << (6 * i) for i in range(42))]
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint8).reshape(-1, 32)


# ---- the compiled gfx950 code of a source file, for the ISA tests (hipcc -S, no GPU needed) ----------------------------------------------------------
CSRC = os.path.join(ROOT, "curve25519-dalek_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def device_asm(tmp_path_factory, name):
    """-> the lines of the gfx950 assembly of csrc/<name>.hip (release flags, device code only)"""
    out = tmp_path_factory.mktemp("isa") / (name + ".s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out), os.path.join(CSRC, name + ".hip")],
                   check=True, capture_output=True, timeout=900)
    return open(out).read().split("\n")


def asm_functions(lines, pattern):
    """-> {mangled name: body lines after the label} for every function whose label matches `pattern`"""
    out = {}
    for i, l in enumerate(lines):
        m = re.match(r"^(" + pattern + r"\S*):", l)
        if m:
            end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
            out[m.group(1)] = lines[i + 1:end]
    return out


def asm_ops(body):
    """-> the opcodes of the instructions in `body`"""
    return [x.split()[0] for x in body if re.match(r"^\s+[a-z]", x)]


# ---- kernels of an assembly file and where their conditional branches come from (tests/test_ct_isa_secret_paths.py) ------------------------------------------
def demangle_kernel(sym):
    """'_ZN6c2551910k_var_baseILi0ELb1ELb1EEEvPKh...' -> 'k_var_base<0, true, true>' (the base name and integer / bool template arguments: all the library uses);
    None if `sym` is not of that form"""
    m = re.match(r"^_Z(N6c25519)?(\d+)", sym)
    if not m:
        return None
    a = m.end()
    name, rest = sym[a:a + int(m.group(2))], sym[a + int(m.group(2)):]
    if not rest.startswith("I"):
        return name
    args, rest = [], rest[1:]
    while not rest.startswith("E"):
        t = re.match(r"^L([a-z])(n?)(\d+)E", rest)
        if not t:
            return None
        v = int(t.group(3)) * (-1 if t.group(2) else 1)
        args.append(("true" if v else "false") if t.group(1) == "b" else str(v))
        rest = rest[t.end():]
    return "%s<%s>" % (name, ", ".join(args))


def asm_kernels(lines):
    """-> {mangled name: (body lines, private segment bytes)} of every KERNEL of an assembly file (the .amdhsa_kernel directives name them)"""
    text = "\n".join(lines)
    priv = {m.group(1): int(m.group(2)) for m in re.finditer(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)", text)}
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    assert names and sorted(names) == sorted(priv), (sorted(set(names) ^ set(priv)))
    out = {}
    for n in names:
        body = asm_functions(lines, re.escape(n) + r"(?=:)")
        assert list(body) == [n], (n, list(body))
        out[n] = (body[n], priv[n])
    return out


_SCC_WRITERS = re.compile(r"^s_(cmp|cmpk|bitcmp\d|and|or|xor|andn2|orn2|nand|nor|xnor|not|add|sub|addc|subb|addk|lshl|lshr|ashr|bfe|min|max|abs|absdiff|lshl\d_add|wqm|quadmask|bcnt\d)_|^s_\w+_saveexec_")


def _regs(operand):
    """the scalar registers an operand names -> set of ('s', k) / ('vcc',) / ('exec',); empty for literals, VGPRs are reported as ('v',)"""
    o = operand.strip()
    m = re.match(r"^s\[(\d+):(\d+)\]$", o)
    if m:
        return {("s", k) for k in range(int(m.group(1)), int(m.group(2)) + 1)}
    m = re.match(r"^s(\d+)$", o)
    if m:
        return {("s", int(m.group(1)))}
    if o in ("vcc", "vcc_lo", "vcc_hi"):
        return {("vcc",)}
    if o in ("exec", "exec_lo", "exec_hi"):
        return {("exec",)}
    if re.match(r"^(v\d+|v\[\d+:\d+\]|a\d+|a\[\d+:\d+\])$", o) or re.match(r"^[|-]*v\d+", o):
        return {("v",)}
    return set()


def _parse(line):
    """'\\ts_and_b64 vcc, exec, s[4:5]' -> ('s_and_b64', ['vcc', 'exec', 's[4:5]']); None for labels, directives, comments"""
    m = re.match(r"^\s+([a-z_0-9]+)\s*(.*)$", line)
    if not m:
        return None
    ops = [x.strip() for x in re.sub(r";.*$", "", m.group(2)).split(",")] if m.group(2).strip() else []
    return m.group(1), [re.sub(r"\s+(offset|glc|slc|nt|sc\d|dst_sel|src\d_sel|row_|quad_perm|bank_mask|bound_ctrl|op_sel|clamp|mul:|div:).*$", "", o) for o in ops if o]


def _writes(op, ops):
    """the scalar registers (and 'scc') an instruction writes"""
    w = set()
    if op.startswith(("s_cmp", "s_bitcmp")):
        return {("scc",)}
    if op.startswith(("s_cbranch", "s_branch", "s_waitcnt", "s_nop", "s_barrier", "s_endpgm", "s_setprio", "s_sleep", "s_set", "s_store", "s_dcache", "s_icache")):
        return w
    if op.startswith("s_") and ops:
        w |= _regs(ops[0])
        if _SCC_WRITERS.match(op):
            w.add(("scc",))
        if "saveexec" in op:
            w.add(("exec",))
    elif op.startswith("v_cmpx"):
        w.add(("exec",))
        if ops:
            w |= _regs(ops[0]) - {("v",)}
    elif op.startswith("v_") and ops:
        w |= _regs(ops[0]) - {("v",)}                       # v_cmp* / v_readfirstlane / v_readlane: an SGPR or vcc destination
        if len(ops) > 1 and re.search(r"_co_|v_div_scale|v_mad_[ui]64", op):
            w |= _regs(ops[1]) - {("v",)}                   # the carry-out of v_add_co / v_subrev_co ... is the second operand
    return w


def branch_origins(body):
    """For every conditional branch of a kernel body -> [(line index, opcode, verdict, witness)] with verdict
      'uniform'  s_cbranch_scc*, or a vcc / exec condition that comes, through scalar instructions only, from values no VGPR ever entered (kernel arguments,
                 constants, scalar counters): the same for every lane and independent of per-lane data;
      'bounds'   the condition is an unsigned ordered v_cmp of a VGPR against a scalar KERNEL ARGUMENT (an s_load result): the item index against n;
      'lane'     anything else: the condition depends on a per-lane value.  `witness` is the vector instruction it comes from.
    A TEXTUAL walk, not a proof: from the branch back to the last writer of its condition register above it in the text, then of that instruction's scalar
    sources, and so on.  Where the branch lies inside a loop (a backward branch below it targets a label at or above it), writers between the branch and that
    backward branch reach it too and are followed as well; the worse verdict wins.  Other control flow is ignored.  Every s_load result counts as a kernel
    argument, also one loaded through a pointer (the kernels here load only their argument block and __constant__ tables with scalar loads)."""
    ins = [_parse(l) for l in body]
    writes = [(_writes(*p) if p else set()) for p in ins]

    labels = {m.group(1): k for k, l in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    loops = []                                              # (label line, backward branch line)
    for k, l in enumerate(body):
        m = re.search(r"s_c?branch\w* (\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), k + 1) <= k:
            loops.append((labels[m.group(1)], k))

    def writers(reg, i):
        """the instructions whose value of `reg` can be live at line i: the last writer above, and every writer below it up to the end of a loop around i"""
        out = []
        for j in range(i - 1, -1, -1):
            if reg in writes[j]:
                out.append(j)
                break
        end = max([b for t, b in loops if t <= i <= b], default=i)
        out += [j for j in range(i + 1, end + 1) if reg in writes[j]]
        return out

    memo, busy = {}, set()
    rank = {"uniform": 0, "arg": 0, "bounds": 1, "lane": 2}

    def origin(reg, i, depth=0):
        """-> ('uniform', None) | ('arg', None) | ('lane' | 'bounds', witness line)"""
        ws = writers(reg, i)
        if not ws:
            return ("uniform", None)                        # set up by the launch (kernel-argument pointer, workgroup id)
        res = [origin_at(reg, j, depth) for j in ws]
        worst = max(res, key=lambda r: rank[r[0]])
        if worst[0] in ("uniform", "arg") and any(r[0] == "uniform" for r in res):
            return ("uniform", None)
        return worst

    def origin_at(reg, j, depth):
        if (reg, j) in memo:
            return memo[(reg, j)]
        if (reg, j) in busy:
            return ("arg", None)                            # a cycle through a loop-carried scalar: decided by its other writers
        busy.add((reg, j))
        res = _origin_at(reg, j, depth)
        busy.discard((reg, j))
        memo[(reg, j)] = res
        return res

    def _origin_at(reg, j, depth):
        op, ops = ins[j]
        res = ("uniform", None)
        if op.startswith("v_"):
            res = ("lane", body[j].strip())
            if re.match(r"^v_cmpx?_(lt|le|gt|ge)_u(32|64)", op):
                srcs = ops[1:] if _regs(ops[0]) - {("v",)} else ops
                sregs = [r for o in srcs for r in _regs(o) if r[0] == "s"]
                if sregs and all(origin(r, j, depth + 1)[0] == "arg" for r in sregs):
                    res = ("bounds", body[j].strip())
        elif op.startswith(("s_load", "s_buffer_load")):
            res = ("arg", None)
        elif depth > 64:
            res = ("lane", "trace too deep: " + body[j].strip())
        else:
            srcs = ops[1:]
            if op.startswith(("s_cmp", "s_bitcmp")):
                srcs = ops
            regs = {r for o in srcs for r in _regs(o)} - {("exec",)}
            if op.startswith(("s_cselect", "s_addc", "s_subb", "s_cmov")):
                regs.add(("scc",))
            if ("v",) in regs:
                res = ("lane", body[j].strip())
            kinds = [origin(r, j, depth + 1) for r in sorted(regs - {("v",)})]
            for k in kinds:
                if k[0] in ("lane", "bounds") and res[0] != "lane":
                    res = k
            if res[0] == "uniform" and kinds and all(k[0] == "arg" for k in kinds) and op.startswith(("s_mov", "s_lshl", "s_lshr", "s_and", "s_add", "s_sub", "s_mul")):
                res = ("arg", None)                         # still a function of kernel arguments alone
        return res

    out = []
    for i, p in enumerate(ins):
        if not p or not p[0].startswith("s_cbranch_"):
            continue
        op = p[0]
        if op.startswith("s_cbranch_scc"):
            out.append((i, op, "uniform", None))
            continue
        reg = ("vcc",) if op.startswith("s_cbranch_vcc") else ("exec",) if op.startswith("s_cbranch_exec") else None
        assert reg, "unknown conditional branch: " + body[i]
        kind, wit = origin(reg, i)
        out.append((i, op, "uniform" if kind == "arg" else kind, wit))
    return out
