"""The device z-mode's coefficients against their specification (tests/pyref.py device_zs: hashlib BLAKE2b, written from include/c25519_hip.h) at every shape of
the hash tree -- tests/pyref_ztree.py has the launch geometry and the sizes, tests/test_ztree_shapes_host.py shows that the sizes reach every class of it:

  the launch chain   k_ztree_first / k_ztree_block (five levels per launch, then the tail) / k_zderive, through c25519_debug_batch_zs (z_mode 1)
  the host copy      ztree_host_zs (z_mode 2)
  the segment tree   k_mid_vseg_ztree inside one ed25519_verify_batch_segments_dev call whose segments have every length 1 .. 1023, read from the call's workspace

Every comparison is of bytes.  The z_i only have to be nonzero for a verdict to come out right, so no verdict shows a tree that skips a child or tags a level
with the wrong count; these comparisons do."""
import hashlib

import numpy as np
import pytest

import pyref
import pyref_ztree as Z

pytestmark = pytest.mark.gpu

BIG = 65537                                                  # from here on every size is a case of its own
SMALL = tuple(n for n in Z.SIZES if n < BIG)
HOST_SIZES = tuple(range(1, 131)) + (4097, 20481)


@pytest.fixture(scope="module")
def eng():
    import curve25519_dalek_amd as pkg
    return pkg.Engine(0)


def _inputs(n, seed):
    """n seeded (message of 0 .. 5 bytes, 64 signature bytes, 32 key bytes) and their SHA-512(R || A || M): the tree absorbs s verbatim and the hash mod l, so
    the signatures need not verify"""
    rng = np.random.default_rng(seed)
    sb, kb, mb = rng.bytes(64 * n), rng.bytes(32 * n), rng.bytes(5 * n)
    lens = rng.integers(0, 6, n).tolist()
    S = [sb[64 * i:64 * i + 64] for i in range(n)]
    K = [kb[32 * i:32 * i + 32] for i in range(n)]
    M = [mb[5 * i:5 * i + ln] for i, ln in enumerate(lens)]
    hr = [hashlib.sha512(s[:32] + k + m).digest() for s, k, m in zip(S, K, M)]
    return M, S, K, hr


@pytest.fixture(scope="module")
def small_pool():
    return _inputs(max(max(SMALL), max(HOST_SIZES)), 4100)


def _compare(got, want, n):
    """-> None, or what differs: a tree error changes every row, a k_zderive error single rows"""
    assert got.shape == (n, 16) and len(want) == n
    w = np.frombuffer(b"".join(want), np.uint8).reshape(n, 16)
    diff = np.nonzero((got != w).any(axis=1))[0]
    if diff.size == 0:
        return None
    return {"n": n, "rows that differ": int(diff.size), "first": int(diff[0]), "shape": Z.tree_shape(n)}


def _summary(wrong):
    return "%d sizes differ: n = %s; the first: %s" % (len(wrong), [w["n"] for w in wrong], wrong[0])


def _chain_case(eng, M, S, K, hr, n, z_mode):
    return _compare(eng.debug_batch_zs(M[:n], S[:n], K[:n], z_mode), pyref.device_zs(hr[:n], [s[32:] for s in S[:n]]), n)


def test_launch_chain_small_sizes(eng, small_pool):
    M, S, K, hr = small_pool
    assert len(SMALL) > 170 and max(SMALL) == 20481
    wrong = [w for w in (_chain_case(eng, M, S, K, hr, n, 1) for n in SMALL) if w]
    assert wrong == [], _summary(wrong)


@pytest.mark.parametrize("n", [n for n in Z.SIZES if n >= BIG])
def test_launch_chain_large_size(eng, n):
    M, S, K, hr = _inputs(n, n)
    wrong = _chain_case(eng, M, S, K, hr, n, 1)
    assert wrong is None, wrong


def test_host_copy(eng, small_pool):
    """ztree_host_zs serves batches of at most 128 signatures in production; the loops it shares with nothing else are checked past that too"""
    M, S, K, hr = small_pool
    wrong = [w for w in (_chain_case(eng, M, S, K, hr, n, 2) for n in HOST_SIZES) if w]
    assert wrong == [], _summary(wrong)


# ---- the segment tree, in the pipeline itself ---------------------------------------------------------------------------------------------------
def test_segment_tree_every_length_in_one_call(orc):
    """One call in the device z-mode whose 1023 segments have every length 1 .. 1023 once, shuffled: 523 776 honest signatures, 1023 rows of tree states, every
    number of leaf nodes 1 .. 256 and leaf rounds 1 .. 4 of the wave.  Every status is OK (which any nonzero z_i give); then the z_i the call left in its workspace
    -- tmp_c2: hram (n x 64, rounded up to 256) | 256 bytes | z16, the layout at vseg_run in csrc/verify_seg.hip; no later stage of the call touches tmp_c2 --
    must be device_zs of each segment alone.  The hram region is compared with hashlib first: that authenticates the layout."""
    import torch
    import curve25519_dalek_amd as pkg
    lens = np.arange(1, pkg.engine.VERIFY_SEGMENT_MAX + 1)
    np.random.default_rng(1023).shuffle(lens)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    n = int(off[-1])
    assert n == 523776 and len(lens) == 1023 and sorted(lens.tolist()) == list(range(1, 1024))
    g = torch.Generator(device="cuda"); g.manual_seed(523776)
    seeds = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g)
    mlen = np.array([(5 * i) % 23 for i in range(n)], np.int64)
    moff = np.zeros(n + 1, np.int64); moff[1:] = np.cumsum(mlen)
    dm = torch.randint(0, 256, (int(moff[-1]) + 16,), dtype=torch.uint8, device="cuda", generator=g)[:int(moff[-1])]
    dmoff = torch.from_numpy(moff).cuda()
    eng = pkg.Engine(0)                                      # a context of its own: its workspaces hold this call and nothing else
    try:
        dp, ds = eng.sign_batch_t(seeds, dm, dmoff)
        mb, sb, kb = dm.cpu().numpy().tobytes(), ds.cpu().numpy().tobytes(), dp.cpu().numpy().tobytes()
        for i in (0, 1, n // 3, n // 2, n - 2, n - 1):       # (the signer is pinned byte-exact elsewhere; the oracle on a handful)
            assert orc.ed25519_verify(kb[32 * i:32 * i + 32], mb[int(moff[i]):int(moff[i + 1])], sb[64 * i:64 * i + 64]) == 0, i
        assert eng.verify_batch_segments_plan(off)[:2] == (1023, 0)
        st = eng.verify_batch_segments_t(dm, dmoff, ds, dp, off, 1).cpu().numpy()
        ws = eng.workspaces()["tmp_c2"]
    finally:
        eng.close()
    assert st.shape == (1023,) and not st.any(), [(int(lens[j]), int(st[j])) for j in np.nonzero(st)[0][:20]]
    hr = [hashlib.sha512(sb[64 * i:64 * i + 32] + kb[32 * i:32 * i + 32] + mb[int(moff[i]):int(moff[i + 1])]).digest() for i in range(n)]
    c_h = (n * 64 + 255) // 256 * 256
    z0 = c_h + 256
    assert ws.size >= z0 + n * 16, "tmp_c2 is smaller than hram | 256 | z16: the layout at vseg_run (csrc/verify_seg.hip) has moved"
    bad = np.nonzero((ws[:n * 64].reshape(n, 64) != np.frombuffer(b"".join(hr), np.uint8).reshape(n, 64)).any(axis=1))[0]
    assert bad.size == 0, ("tmp_c2 does not begin with SHA-512(R || A || M) of every signature: the layout at vseg_run (csrc/verify_seg.hip) has moved, "
                           "or k_hram is wrong", int(bad.size), int(bad[0]))
    z = ws[z0:z0 + n * 16].reshape(n, 16)
    wrong = []
    for j, ln in enumerate(lens.tolist()):
        a = int(off[j])
        w = _compare(z[a:a + ln], pyref.device_zs(hr[a:a + ln], [sb[64 * i + 32:64 * i + 64] for i in range(a, a + ln)]), ln)
        if w:
            wrong.append((ln, j, w["rows that differ"], w["first"]))
    agree = sorted(set(lens.tolist()) - {w[0] for w in wrong})
    assert wrong == [], ("%d lengths differ; (length, segment, rows that differ, first): %s ...; lengths that agree: %s%s"
                         % (len(wrong), sorted(wrong)[:12], agree[:40], " ..." if len(agree) > 40 else ""))
