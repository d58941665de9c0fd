"""Every kernel of the library is classified as secret-handling or public, and the secret-handling ones are checked whole on the COMPILED code
(hipcc -S for gfx950, no GPU needed).

What is checked for a SECRET kernel (and, beside the older test that stays its authority, for a SECRET_LOOP_ONLY one): no calls beyond the listed ones, a
private segment of zero bytes (a block buffer in scratch holds the signing prefix where nothing can wipe it: k_sign_nonce did, until sha512_stream wrote
its block through selects), and every conditional branch either uniform (util.branch_origins: s_cbranch_scc*, or a vcc / exec condition that comes, as
far as a textual walk through the scalar instructions shows, from values no VGPR entered), a bounds exit (the item index against the kernel argument n),
or lane-dependent and then PINNED: tests/golden/ct_isa_secret_paths.json holds, per kernel, how many branches each vector instruction (its opcode and
operand classes: the source condition) feeds, and the kernel's row says why those conditions are public.  The counts are exact: one new lane-dependent
branch, or one that trades a length compare for another kind of compare, fails the test.  They move with the compiler; after checking that every new
witness is still a length, an index or a counter, regenerate the file with  python tests/test_ct_isa_secret_paths.py --regen.

What is NOT checked here: addresses.  That no load address derives from a secret cannot be proven from the text in general; the loop-level load
assertions of tests/test_ct_isa.py remain what they are, and this module claims nothing about addresses outside those loops."""
import json
import os
import re
import sys
from collections import Counter
from concurrent.futures import ThreadPoolExecutor

import pytest

from util import CSRC, HIPCC, asm_kernels, asm_ops, branch_origins, demangle_kernel, device_asm

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")

SECRET, SECRET_LOOP_ONLY, PUBLIC = "SECRET", "SECRET_LOOP_ONLY", "PUBLIC"
_VT = "a non-constant-time instantiation: reached only through FLAG_VARTIME_TABLES contexts and the *_vartime* entry points, which declare their scalars public"
_LEN = ("message-length control flow of the SHA-512 absorber (lengths, offsets and alignment are public; the prefix and the hash state only pass through selects "
        "and arithmetic) and the round counter of its compression, kept in a VGPR inside those loops")
# (pattern on the demangled name, class, reason / the older test that covers it, {lane: exact count of lane-dependent branches, bounds: distinct index
#  compares, calls: allowed call instructions, why: why the lane-dependent branches pinned in GOLDEN for the row's kernels are public})
TABLE = [
    # ---- signing and key generation (single.hip) ----
    (r"k_expand_seed", SECRET, "the seed and its SHA-512 expansion", {}),
    (r"k_sign_nonce", SECRET, "the prefix and the nonce", {"why": _LEN}),
    (r"k_sign_nonce_dom", SECRET, "the prefix and the nonce (Ed25519ph)", {"why": _LEN}),
    (r"k_sign_finish", SECRET, "S = r + k a: the key and the nonce", {}),
    (r"k_clamp", SECRET, "raw secret bytes -> clamped scalars", {}),
    (r"k_var_base<\d, (true|false), true>", SECRET_LOOP_ONLY, "test_ct_isa.test_variable_base_scan_has_no_data_dependent_branch",
     {"why": "loop counters the compiler keeps in VGPRs: the table build (j = 2..8), the 64 digits and the nine-entry scan; none is compared with scalar data"}),
    (r"k_var_base<\d, (true|false), false>", PUBLIC, _VT, {}),
    (r"k_p40_to_raw", SECRET, "carries secret * P", {}),
    (r"k_p40_add_to_p32", SECRET, "carries secret * P", {}),
    (r"k_(hram_reduce|strict_checks|verdict|place_R|fill_order|flag_identity_enc|small_order<\d>)", PUBLIC,
     "per-signature verification and order checks: signatures, keys, messages and the points checked are public (R in k_place_R is half of the signature)", {}),
    # ---- fixed base, X25519, decompression (kernels.hip) ----
    (r"k_x25519", SECRET_LOOP_ONLY, "test_ct_isa.test_ladder_loop_has_no_data_dependent_branch", {}),
    (r"k_mul_base_ctp<5, \d+, \d, true, (true|false)>", SECRET_LOOP_ONLY, "test_ct_isa.test_fixed_base_cross_lane_fetch_loop",
     {"why": "lane and item indices against the batch size and the split point (thread position, not data), and wave-uniform values read with v_readfirstlane from the staged table header"}),
    (r"k_mul_base_ctp<5, 1024, \d, false, (true|false)>", SECRET_LOOP_ONLY, "test_ct_isa.test_fixed_base_cross_lane_fetch_loop",
     {"spill": True, "why": "thread and item indices against the batch size while the table is staged"}),
    (r"k_mul_base_ct_split<\d+, \d>", SECRET_LOOP_ONLY, "test_ct_isa.test_fixed_base_split_kernel_scan_is_the_same",
     {"why": "thread indices: which half of a scalar's windows a thread works on, the staging loop of the table, and the pairwise combination of the halves"}),
    (r"k_mul_base<5, 1024, \d, true>", SECRET_LOOP_ONLY, "test_ct_isa.test_fixed_base_scan_reads_every_entry_without_a_branch",
     {"bounds": 2, "why": "the thread index against the table size in the LDS staging loop"}),
    (r"k_mul_base<\d, \d+, \d, false>", PUBLIC, _VT, {}),
    (r"k_mul_base_wide<\d>", PUBLIC, _VT, {}),
    (r"k_mul_base_comb<\d+, \d>", PUBLIC, _VT + " (and builds the context's own tables from public multiples of B)", {}),
    (r"k_(decompress_edwards|decompress_ristretto|prep_compressed<\d>|prep_compressed_keys_and_r)", PUBLIC, "decompression of wire points: public encodings", {}),
    # ---- finishing kernels (finish.hip, extra.hip, capi.hip) ----
    (r"k_ratio_p32<16, \d>", SECRET, "produces the X25519 shared secret",
     {"bounds": 3, "why": "the counter of the strided batch-inversion loop, kept in a VGPR"}),
    (r"k_compress_p32<16>", SECRET, "carries secret * P",
     {"bounds": 5, "why": "the chunk counters of the strided batch-inversion loops, kept in VGPRs (compared with constants, not with data)"}),
    (r"k_compress_raw", SECRET, "carries secret * P (batches below 4096 points)", {}),
    (r"k_compress_ristretto", SECRET, "carries secret * P (Ristretto outputs)", {}),
    (r"k_raw_to_p32", SECRET, "carries secret * P", {}),
    (r"k_sum_p40", SECRET, "partial sums of the constant-time MSM", {"why": "threadIdx.x == 0 stores the wave's sum"}),
    (r"k_scalar_invert<16>", SECRET, "secret scalars and their inverses",
     {"bounds": 3, "why": "the counter of the strided batch-inversion loop, kept in a VGPR"}),
    (r"k_nonzero32", SECRET, "reads the shared secrets (was_contributory)", {}),
    (r"k_double_compress<16>", PUBLIC, "double_and_compress_batch takes public points (no secret-taking entry point reaches it)", {}),
    (r"k_prep_small_verify", PUBLIC, "verify_batch: signatures and keys", {}),
    (r"k_selftest_(field<\d>|point<\d>|scalar)", PUBLIC, "diagnostics: device self-tests on test vectors", {}),
    (r"k_probe_\w+(<.*>)?", PUBLIC, "diagnostics: instruction-rate probes, no inputs", {}),
    # ---- the newest files: whole-kernel tests of their own stay the authority ----
    (r"k_mont_(mul|mul_bits|to_edwards_prep|to_edwards<\d, (true|false)>)", SECRET_LOOP_ONLY, "test_ct_isa_montgomery (whole kernel)", {}),
    (r"k_(lizard_encode|lizard_decode|map_to_curve_inverse)<\d>", SECRET_LOOP_ONLY, "test_ct_isa_lizard (whole kernel)",
     {"calls": 1, "why": "the out-of-line field function of the <0> instantiations, which test_ct_isa_lizard checks"}),
    (r"k_ristretto_(from_uniform|map)<\d>", SECRET_LOOP_ONLY, "test_ct_isa_h2c (whole kernel)",
     {"calls": 1, "why": "the out-of-line field function, which test_ct_isa_h2c checks"}),
    (r"k_(ristretto_hash<\d>|edwards_h2c<(true|false), \d>)", PUBLIC,
     "hash_from_bytes / hash_to_curve of caller messages: control flow follows the public message and DST lengths; test_ct_isa_h2c covers the map itself", {}),
    (r"k_(group_elem<.*>|group_eq<.*>|group_any_bad|seg_sum<\d>|seg_finish<\d>|seg_keys)", PUBLIC,
     "the group law on caller points: no scalar enters; test_ct_isa_group asserts its select-only posture all the same", {}),
    # ---- verification, the vartime MSM and its sort / reduce kernels ----
    (r"k_(hram|hram_dom|hram_mod_l|ztree_first|ztree_block|zderive|z_expand|batch_scalars|bsum_finish|apply_sign|add_point_counters)", PUBLIC,
     "verify_batch: signatures, keys, messages and the batch coefficients derived from them are public", {}),
    (r"k_(accumulate|accumulate_long|mid_\w+(<\d>)?|small_cols|small_reduce<\d+>|reduce_\w+|long_combine|long_segments|prep_basepoint|prep_raw2<.*>|publish|record_sum|slot_init)", PUBLIC,
     "the vartime MSM (msm_vartime, verify_batch): public scalars by contract", {}),
    (r"k_(bin_totals|order_place<\d+>|part2g<.*>|sweep_local<\d+>|digits|digits_merged|hist|merged_table|order_hist|order_scan|order_scatter|part1|part2|part_hist|part_scan|"
     r"scan_buckets|scan_chunks|scatter|scatter_sliced)", PUBLIC, "the bucket sort of the vartime MSM: digits of public scalars", {}),
]


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ct_isa_secret_paths.json")


def witnesses(body):
    """{source condition: number of lane-dependent branches it feeds}: the vector instruction util.branch_origins names, register numbers and literals as N"""
    return dict(Counter(re.sub(r"\d+", "N", w) for _, _, kind, w in branch_origins(body) if kind == "lane"))


def release_sources():
    """the .hip files libc25519hip.so is linked from: the OBJS of csrc/Makefile"""
    m = re.search(r"^OBJS\s*=\s*(.+)$", open(os.path.join(CSRC, "Makefile")).read(), flags=re.M)
    names = [o[:-2] for o in m.group(1).split() if o.endswith(".o")]
    assert len(names) >= 18 and all(os.path.exists(os.path.join(CSRC, n + ".hip")) for n in names), names
    return names


@pytest.fixture(scope="module")
def library_kernels(tmp_path_factory):
    """{demangled kernel: (file, body, private segment bytes)} of every kernel of the release library; each file compiled once, four at a time"""
    names = release_sources()
    with ThreadPoolExecutor(max_workers=4) as pool:
        asms = list(pool.map(lambda n: device_asm(tmp_path_factory, n), names))
    return collect(dict(zip(names, asms)))


def collect(asm_by_file):
    out = {}
    for f, lines in asm_by_file.items():
        for sym, (body, priv) in asm_kernels(lines).items():
            d = demangle_kernel(sym)
            assert d and d.startswith("k_"), "kernel %s of %s.hip: the name does not demangle to k_*" % (sym, f)
            assert d not in out, d
            out[d] = (f, body, priv)
    return out


def classify(kernels):
    """-> ({kernel: row}, errors)"""
    rows, errs, used = {}, [], set()
    for k in sorted(kernels):
        hit = [i for i, r in enumerate(TABLE) if re.fullmatch(r[0], k)]
        if len(hit) != 1:
            errs.append("kernel %s (%s.hip) is matched by %d rows of TABLE: classify it as SECRET, SECRET_LOOP_ONLY or PUBLIC in tests/test_ct_isa_secret_paths.py"
                        % (k, kernels[k][0], len(hit)))
            continue
        rows[k] = TABLE[hit[0]]
        used.add(hit[0])
    errs += ["row %r of TABLE matches no kernel of the library: remove or correct it" % TABLE[i][0] for i in range(len(TABLE)) if i not in used]
    return rows, errs


def check_secret(name, body, priv, info, pinned=None):
    """-> the violations of the whole-kernel rule"""
    errs = []
    ops = asm_ops(body)
    calls = sum(o.startswith(("s_swappc", "s_setpc", "s_call")) for o in ops)
    if calls > info.get("calls", 0):
        errs.append("%s: %d call instructions (allowed: %d)" % (name, calls, info.get("calls", 0)))
    if info.get("spill"):
        # the one allowance: test_ct_isa.test_fixed_base_cross_lane_fetch_loop accepts at most 2 scratch_load inside the window loop of these instantiations, the
        # reloads of the "six words" its comment says they spill.  Whole-kernel, the same thing is a private segment of at most those six words (24 bytes), every
        # access at a compile-time offset (no VGPR address: nothing a digit could index).  Neither is wider than the other; today both counts are zero.
        dyn = [l.strip() for l in body if re.match(r"^\s+scratch_(load|store)", l) and not re.search(r"\boff\b.*\boff\b|, off\b", l)]
        if priv > 24 or dyn:
            errs.append("%s: private segment %d bytes (allowed: six spilled words at compile-time offsets) %s" % (name, priv, dyn[:3]))
    elif priv != 0 or any(o.startswith("scratch_") for o in ops):
        errs.append("%s: private segment of %d bytes / scratch traffic: secrets in memory nothing can wipe" % (name, priv))
    br = branch_origins(body)
    bounds = {w for _, _, kind, w in br if kind == "bounds"}
    got, want = witnesses(body), (pinned or {})
    if got != want:
        diff = {k: (want.get(k, 0), got.get(k, 0)) for k in sorted(set(got) | set(want)) if got.get(k, 0) != want.get(k, 0)}
        errs.append("%s: lane-dependent branches differ from the pinned ones, {source condition: (pinned, compiled)} = %s" % (name, diff))
    if got and not info.get("why"):
        errs.append("%s: has lane-dependent branches and its row gives no reason why they are public" % name)
    if len(bounds) > info.get("bounds", 1):
        errs.append("%s: %d distinct index compares feed branches, the row allows %d: %s" % (name, len(bounds), info.get("bounds", 1), sorted(bounds)))
    return errs


def test_every_kernel_is_classified(library_kernels):
    rows, errs = classify(library_kernels)
    assert not errs, "\n".join(errs)
    for k, r in rows.items():
        assert r[1] in (SECRET, SECRET_LOOP_ONLY, PUBLIC) and len(r[2]) > 10, r
    must = ["k_expand_seed", "k_sign_nonce", "k_sign_nonce_dom", "k_sign_finish", "k_clamp", "k_scalar_invert<16>", "k_x25519", "k_ratio_p32<16, 0>", "k_compress_p32<16>",
            "k_compress_raw", "k_raw_to_p32", "k_p40_to_raw", "k_p40_add_to_p32", "k_sum_p40", "k_var_base<0, false, true>", "k_mul_base<5, 1024, 0, true>",
            "k_mul_base_ct_split<256, 0>", "k_mul_base_ctp<5, 1024, 0, true, true>"]
    for k in must:
        assert k in rows and rows[k][1] != PUBLIC, k


def test_secret_kernels_whole(library_kernels):
    rows, errs = classify(library_kernels)
    assert not errs, "\n".join(errs)
    pinned = json.load(open(GOLDEN))
    bad = ["%s is pinned in %s and is no secret kernel of the library" % (k, GOLDEN) for k in pinned if k not in rows or rows[k][1] == PUBLIC]
    for k, r in rows.items():
        if r[1] != PUBLIC:
            _, body, priv = library_kernels[k]
            bad += check_secret(k, body, priv, r[3], pinned.get(k))
    assert not bad, "\n".join(bad)


# ---- the classifier itself, on hand-written snippets ----------------------------------------------------------------------------------------------------
def _verdicts(text):
    return [(op, kind) for _, op, kind, _ in branch_origins(text.split("\n"))]


def test_branch_origins_uniform_sgpr_pattern():
    assert _verdicts("""
	s_load_dwordx2 s[4:5], s[0:1], 0x8
	s_cmp_lg_u32 s12, 0
	s_cselect_b64 s[14:15], -1, 0
	v_add_u32_e32 v1, v2, v3
	s_and_b64 vcc, exec, s[14:15]
	s_cbranch_vccz .LBB0_7
	s_cmp_eq_u32 s12, 80
	s_cbranch_scc0 .LBB0_3""") == [("s_cbranch_vccz", "uniform"), ("s_cbranch_scc0", "uniform")]


def test_branch_origins_v_cmp_fed():
    assert _verdicts("""
	v_cmp_eq_u32_e64 s[2:3], 3, v17
	s_and_b64 vcc, exec, s[2:3]
	s_cbranch_vccnz .LBB0_9
	v_cmp_ne_u32_e32 vcc, 0, v5
	s_and_saveexec_b64 s[6:7], vcc
	s_cbranch_execz .LBB0_11""") == [("s_cbranch_vccnz", "lane"), ("s_cbranch_execz", "lane")]


def test_branch_origins_counter_in_a_vgpr():
    assert _verdicts("""
	v_subrev_co_u32_e32 v80, vcc, 1, v80
	s_and_b64 vcc, exec, vcc
	s_cbranch_vccnz .LBB0_2""") == [("s_cbranch_vccnz", "lane")]


def test_branch_origins_bounds_exit():
    assert _verdicts("""
	s_load_dwordx2 s[4:5], s[0:1], 0x10
	v_cmp_gt_u64_e32 vcc, s[4:5], v[0:1]
	s_and_saveexec_b64 s[2:3], vcc
	s_cbranch_execz .LBB0_66
	v_readfirstlane_b32 s9, v4
	s_cmp_eq_u32 s9, 0
	s_cselect_b64 s[10:11], -1, 0
	s_and_b64 vcc, exec, s[10:11]
	s_cbranch_vccz .LBB0_5""") == [("s_cbranch_execz", "bounds"), ("s_cbranch_vccz", "lane")]


def regen(asm_by_file):
    kernels = collect(asm_by_file)
    rows, errs = classify(kernels)
    assert not errs, errs
    pinned = {k: witnesses(kernels[k][1]) for k in sorted(rows) if rows[k][1] != PUBLIC}
    json.dump({k: v for k, v in pinned.items() if v}, open(GOLDEN, "w"), indent=1, sort_keys=True)


if __name__ == "__main__" and "--regen" in sys.argv:
    import pathlib
    import tempfile

    class _Tmp:
        def mktemp(self, name):
            return pathlib.Path(tempfile.mkdtemp(prefix=name))
    regen({n: device_asm(_Tmp(), n) for n in release_sources()})
