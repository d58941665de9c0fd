"""The launch geometry of the device z-mode's hash tree (csrc/verify.hip zchain_enqueue: k_ztree_first, k_ztree_block five levels per launch, the single-block
tail, k_zderive), restated in plain Python -- no code shared with csrc/ -- and a second evaluation of the tree in the kernels' shape: blocks of 1024 nodes, five
levels per block through two buffers, then the tail.  tests/pyref.py device_zs is the specification (written from include/c25519_hip.h, level by level over
whole lists); this file says which code paths a batch size takes, from which the tests derive their sizes.

  tree_shape(n)           what a batch of n signatures runs through: see the keys below
  classes(n)              the same as a set of class names; ALL_CLASSES is what SIZES has to reach, UNREACHABLE what no single pass can
  kernel_shaped_zs        the z_i evaluated block by block as k_ztree_block does it (hashlib BLAKE2b)
"""
import hashlib

L = 2**252 + 27742317777372353535851937790883648493
BLOCK = 1024                                                 # nodes a block of k_ztree_block owns: 4^5
INNER = 5                                                    # levels per block launch
VERIFY_PASS_MAX = 1572864                                    # csrc/verify.hip: the most signatures one pass (one tree) ever holds
TAG = b"c25519-hip/verify_batch/z-tree/v5"


def _last_children(m):
    """children of the LAST node of the level above a level of m nodes (1 .. 4)"""
    return m - 4 * ((m + 3) // 4 - 1)


def tree_shape(n):
    """n signatures -> dict:
      n_mod_4        signatures of the last leaf node are n_mod_4 or 4
      leaves         nodes k_ztree_first writes (level 0)
      block_launches 5-level launches of k_ztree_block
      blocks         [per launch: (blocks, nodes held by the last block)]
      last_block     per launch: "1", "partial" or "full"
      inner_children [per launch: the children (1 .. 4) of the last node at each of its five levels]
      tail_in        nodes entering the single-block tail (1 .. 1024) and tail_class: "1", "2-4", "5-1023", "1024"
      tail_children  the children of the last node at every tail level (empty when tail_in is 1)
      top_level      index of the root's level (0 = the root is a leaf node)"""
    assert n >= 1
    mm = (n + 3) // 4
    out = {"n": n, "n_mod_4": n % 4, "leaves": mm, "blocks": [], "last_block": [], "inner_children": []}
    level = 1
    while mm > BLOCK:
        mo = (mm + BLOCK - 1) // BLOCK
        last = mm - BLOCK * (mo - 1)
        out["blocks"].append((mo, last))
        out["last_block"].append("1" if last == 1 else "full" if last == BLOCK else "partial")
        m, ch = mm, []
        for _ in range(INNER):
            ch.append(_last_children(m))
            m = (m + 3) // 4
        assert m == mo
        out["inner_children"].append(ch)
        mm = mo
        level += INNER
    out["block_launches"] = len(out["blocks"])
    out["tail_in"] = mm
    out["tail_class"] = "1" if mm == 1 else "2-4" if mm <= 4 else "5-1023" if mm < BLOCK else "1024"
    ch = []
    while mm > 1:
        ch.append(_last_children(mm))
        mm = (mm + 3) // 4
        level += 1
    out["tail_children"] = ch
    out["top_level"] = level - 1
    return out


def classes(n):
    s = tree_shape(n)
    c = {"n%%4=%d" % s["n_mod_4"], "launches=%d" % s["block_launches"], "tail_in=" + s["tail_class"], "top=%d" % s["top_level"]}
    for lb, ch in zip(s["last_block"], s["inner_children"]):
        c.add("last_block=" + lb)
        c |= {"inner%d:children=%d" % (lv, k) for lv, k in enumerate(ch)}
    c |= {"tail:children=%d" % k for k in s["tail_children"]}
    return c


ALL_CLASSES = ({"n%%4=%d" % r for r in range(4)} | {"launches=0", "launches=1"} | {"last_block=" + v for v in ("1", "partial", "full")}
               | {"inner%d:children=%d" % (lv, k) for lv in range(INNER) for k in (1, 2, 3, 4)}
               | {"tail_in=" + v for v in ("1", "2-4", "5-1023", "1024")} | {"tail:children=%d" % k for k in (1, 2, 3, 4)} | {"top=%d" % t for t in range(11)})
# two block launches: more than 1024 * 1024 leaf nodes, i.e. more than 4 194 304 signatures in one pass -- beyond VERIFY_PASS_MAX, so no call builds such a tree
UNREACHABLE = {"launches=2"}

SIZES = tuple(sorted(set(range(1, 131)) | {255, 256, 257, 1000, 1023, 1024, 1025} | set(range(4093, 4102)) | {4104, 4105, 4113, 4116, 4117}
                     | {4132, 4161, 4164, 4165, 4228, 4353, 4356, 4357, 4612}
                     | {5121, 5124, 5125, 6145, 7169, 8188, 8192, 8193, 8196, 8197, 12289}
                     | {16385, 20481, 65537, 262147, 2**20 + 1, 3 * 2**19}))


# ---- the tree as the kernels evaluate it ----------------------------------------------------------------------------------------------------------
def _node(n, level, count, data):
    """BLAKE2b-256(TAG(level, inputs of the level, batch size) || data): the tag block is the string, zeros, then three little-endian u64"""
    blk = TAG + bytes(104 - len(TAG)) + level.to_bytes(8, "little") + count.to_bytes(8, "little") + n.to_bytes(8, "little")
    return hashlib.blake2b(blk + data, digest_size=32).digest()


def _level_counts(n):
    """inputs of level 0, 1, ..: n signatures, then the nodes of the level below"""
    c = [n]
    while c[-1] > 1 or len(c) == 1:
        c.append((c[-1] + 3) // 4)
    return c


ZERO = bytes(32)


def _block(n, counts, nodes, m_in, base, level, nlev):
    """one block of k_ztree_block: the 1024 nodes from `base` of a level of m_in nodes (absent = zero), reduced for nlev levels or until the LEVEL has one node.
    The global counts (m, gbase) decide which children exist and which nodes are computed; a slot nobody wrote keeps what the buffer held."""
    cur = [nodes[base + i] if base + i < m_in else ZERO for i in range(BLOCK)]
    nxt = [None] * (BLOCK // 4)                              # (None: never written -- reading one is an error of the model or of the kernel)
    m, gbase, cnt = m_in, base, BLOCK
    for _ in range(nlev):
        if m <= 1:
            break
        mo, gb, co = (m + 3) // 4, gbase // 4, cnt // 4
        for t in range(co):
            if gb + t < mo:
                kids = [cur[4 * t + ch] if gbase + 4 * t + ch < m else ZERO for ch in range(4)]
                assert None not in kids
                nxt[t] = _node(n, level, counts[level], b"".join(kids))
        cur, nxt = nxt, cur
        m, gbase, cnt, level = mo, gb, co, level + 1
    return cur[0]


def kernel_shaped_zs(hrams, ss):
    """hrams = [H(R||A||M)] (64 bytes each), ss = [s] (32 bytes each) -> the n z_i (16 bytes each), by the launches of zchain_enqueue"""
    n = len(hrams)
    counts = _level_counts(n)
    rec = [(int.from_bytes(h, "little") % L).to_bytes(32, "little") + s for h, s in zip(hrams, ss)]
    mm = (n + 3) // 4
    nodes = [_node(n, 0, n, b"".join(rec[4 * j + r] if 4 * j + r < n else bytes(64) for r in range(4))) for j in range(mm)]      # k_ztree_first
    level = 1
    while mm > BLOCK:
        mo = (mm + BLOCK - 1) // BLOCK
        nodes = [_block(n, counts, nodes, mm, BLOCK * b, level, INNER) for b in range(mo)]
        mm, level = mo, level + INNER
    root = _block(n, counts, nodes, mm, 0, level, 64)        # the tail: one block, until one node is left
    out = []
    for i in range((n + 3) // 4):                            # k_zderive
        d = hashlib.blake2b(root + i.to_bytes(8, "little"), digest_size=64).digest()
        out += [d[16 * q:16 * q + 16] for q in range(4)]
    return out[:n]
