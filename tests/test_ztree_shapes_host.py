"""tests/pyref_ztree.py checked on the host: its sizes reach every class of the z tree's launch geometry, and its block-by-block evaluation of the tree (the shape
of k_ztree_block: 1024 nodes per block, five levels per launch, then the tail) gives the z_i of the specification in tests/pyref.py at every size up to 20 481."""
import hashlib

import numpy as np

import pyref
import pyref_ztree as Z


def test_tree_shape_by_hand():
    s = Z.tree_shape(1)
    assert (s["leaves"], s["block_launches"], s["tail_in"], s["tail_class"], s["tail_children"], s["top_level"]) == (1, 0, 1, "1", [], 0)
    s = Z.tree_shape(5)
    assert (s["n_mod_4"], s["leaves"], s["tail_class"], s["tail_children"], s["top_level"]) == (1, 2, "2-4", [2], 1)
    s = Z.tree_shape(4096)
    assert (s["leaves"], s["block_launches"], s["tail_class"], s["tail_children"], s["top_level"]) == (1024, 0, "1024", [4] * 5, 5)
    # 4097 signatures: 1025 leaf nodes, two blocks, the second holds ONE node and hashes a single child on every level; two nodes enter the tail
    s = Z.tree_shape(4097)
    assert (s["leaves"], s["blocks"], s["last_block"], s["inner_children"], s["tail_in"], s["tail_children"], s["top_level"]) == (1025, [(2, 1)], ["1"], [[1] * 5], 2, [2], 6)
    # 4132 = 4 * 1033: 1033 = 1024 + 9 leaf nodes -> 9, 3, 1, 1, 1 nodes in the last block: the last node of inner level 1 has three children
    s = Z.tree_shape(4132)
    assert (s["blocks"], s["last_block"], s["inner_children"]) == ([(2, 9)], ["partial"], [[1, 3, 1, 1, 1]])
    assert Z.tree_shape(4228)["inner_children"] == [[1, 1, 3, 1, 1]] and Z.tree_shape(4612)["inner_children"] == [[1, 1, 1, 3, 1]]
    s = Z.tree_shape(8192)
    assert (s["blocks"], s["last_block"], s["inner_children"], s["tail_in"]) == ([(2, 1024)], ["full"], [[4] * 5], 2)
    s = Z.tree_shape(3 * 2**19)
    assert (s["leaves"], s["blocks"], s["tail_in"], s["tail_children"], s["top_level"]) == (393216, [(384, 1024)], 384, [4, 4, 4, 2, 2], 10)
    s = Z.tree_shape(2**20 + 1)
    assert (s["blocks"], s["last_block"], s["tail_in"], s["tail_children"], s["top_level"]) == ([(257, 1)], ["1"], 257, [1, 1, 1, 1, 2], 10)


def test_sizes_reach_every_class():
    """each inner level of the block launch with a last node of 1, 2, 3 and 4 children; a last block of one node, a partial and a full one; n % 4 = 0 .. 3; 1, 2 - 4,
    5 - 1023 and 1024 nodes entering the tail; a root on every level 0 .. 10; batches with and without a block launch"""
    assert max(Z.SIZES) <= Z.VERIFY_PASS_MAX and min(Z.SIZES) == 1 and list(Z.SIZES) == sorted(set(Z.SIZES))
    seen = set()
    for n in Z.SIZES:
        seen |= Z.classes(n)
    assert Z.ALL_CLASSES - seen == set(), sorted(Z.ALL_CLASSES - seen)
    assert seen - Z.ALL_CLASSES == set(), sorted(seen - Z.ALL_CLASSES)
    # a second block launch needs more than 1024 * 1024 leaf nodes: more than 4 194 304 signatures in one tree, and a pass holds at most VERIFY_PASS_MAX.
    # The class cannot occur; it is stated here, not covered.
    assert Z.UNREACHABLE == {"launches=2"}
    assert Z.tree_shape(4 * 1024 * 1024)["block_launches"] == 1 and Z.tree_shape(4 * 1024 * 1024 + 1)["block_launches"] == 2
    assert Z.tree_shape(Z.VERIFY_PASS_MAX)["block_launches"] == 1 and Z.VERIFY_PASS_MAX < 4 * 1024 * 1024
    # the ragged block in isolation: sizes whose ONLY node with fewer than four children above the leaves sits inside a block launch
    for lv, n in ((1, 4132), (2, 4228), (3, 4612)):
        assert Z.tree_shape(n)["inner_children"][0][lv] == 3 and n in Z.SIZES
    # every size the segment kernel can see (1 .. 1023) is a tail-only tree of at most 256 leaf nodes and a root on level 4 at most
    assert all(Z.tree_shape(n)["block_launches"] == 0 and Z.tree_shape(n)["leaves"] <= 256 and Z.tree_shape(n)["top_level"] <= 4 for n in range(1, 1024))


def test_block_shaped_evaluation_equals_the_specification():
    rng = np.random.default_rng(20481)
    top = max(n for n in Z.SIZES if n <= 20481)
    assert top == 20481
    hr = [rng.bytes(64) for _ in range(top)]
    ss = [rng.bytes(32) for _ in range(top)]
    for n in (n for n in Z.SIZES if n <= top):
        want = pyref.device_zs(hr[:n], ss[:n])
        got = Z.kernel_shaped_zs(hr[:n], ss[:n])
        assert len(want) == n and got == want, (n, Z.tree_shape(n))
    # the records are (H mod l, s): a hash above l and its reduction give the same tree, any other change another one
    h = (Z.L + 5).to_bytes(64, "little")
    a = Z.kernel_shaped_zs([h] + hr[1:9], ss[:9])
    assert a == Z.kernel_shaped_zs([(5).to_bytes(64, "little")] + hr[1:9], ss[:9]) == pyref.device_zs([h] + hr[1:9], ss[:9])
    assert a != Z.kernel_shaped_zs([(6).to_bytes(64, "little")] + hr[1:9], ss[:9])
    assert hashlib.blake2b(b"", digest_size=32).hexdigest().startswith("0e5751c026e543b2")       # RFC 7693's function under this name
