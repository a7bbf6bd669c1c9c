"""The cases of the deposit tree kept in memory, run against any engine: the host
build (test_deposit_tree_host.py), the library's host-pointer forms and its device forms
(test_deposit_tree_gpu.py).  An engine has
    create(capacity, depth=32) -> tree
and a tree has
    count, capacity
    append(leaves)                          leaves: a list of 32-byte values
    roots(counts) -> [32 bytes per count]
    proofs(indices, k) -> ([32 * depth bytes per index], root)
    close()
each raising ValueError for arguments the engine rejects.  Expected values are
merkle_model.Tree(leaves[:k], 0, depth) -- the reference's get_merkle_root(leaves[:k]) and
get_merkle_proof, which tests/golden/merkle_trees.json pins -- and
tests/golden/deposit_tree_history.json; a model tree is built once per (tree, k) and shared
between the engines.  Every case queries earlier counts after later appends: that is what
separates the tree from one that reads its current boundary nodes."""
import functools
import json
import os

import pytest

import deposit_model
import merkle_model as M

TREE_ID = 310           # the fixture's leaves are tree 300


@functools.lru_cache(maxsize=None)
def leaves(tree_id: int, n: int):
    return tuple(M.leaves_of(tree_id, n))


@functools.lru_cache(maxsize=None)
def model(tree_id: int, k: int, depth: int = 32) -> M.Tree:
    """The tree over the first k leaves of `tree_id` (a prefix of any longer list of its leaves)."""
    return M.Tree(M.leaves_of(tree_id, k), 0, depth)


@functools.lru_cache(maxsize=None)
def fixture():
    with open(os.path.join(M.ROOT, "tests", "golden", "deposit_tree_history.json")) as f:
        return json.load(f)


def split(proof: bytes):
    return [proof[i:i + 32] for i in range(0, len(proof), 32)]


def check_proofs(tree, tree_id, k, indices, depth=32):
    """The proofs of `indices` at count k: the model's siblings and root, and each proof folds
    from its leaf (zero at or above k) to that root by the spec's verify_merkle_branch."""
    m = model(tree_id, k, depth)
    lv = leaves(tree_id, k)
    proofs, root = tree.proofs(list(indices), k)
    assert root == m.root, k
    for i, p in zip(indices, proofs):
        assert split(p) == m.proof(i), (k, i)
        leaf = lv[i] if i < k else M.ZERO
        assert deposit_model.branch_root(leaf, split(p), depth, i) == m.root, (k, i)


# ---------------------------------------------------------------- the fixture
def check_fixture(eng):
    """300 leaves in appends of 7, 64, 1, 184 and 44: the root at every count and the recorded
    proofs, all asked after the last append."""
    fx = fixture()
    lv = leaves(fx["id"], fx["n"])
    with eng.create(1000) as tree:
        at = 0
        for n in (7, 64, 1, 184, 44):
            tree.append(lv[at:at + n])
            at += n
        assert at == fx["n"] == tree.count
        roots = tree.roots(range(1, fx["n"] + 1))
        assert [r.hex() for r in roots] == fx["roots"]
        for p in fx["proofs"]:
            proofs, root = tree.proofs([p["i"]], p["k"])
            assert root.hex() == fx["roots"][p["k"] - 1]
            assert [s.hex() for s in split(proofs[0])] == p["proof"], (p["k"], p["i"])


# --------------------------------------------------- growth by uneven appends
def growth_sizes(W: int):
    sizes = [1, 1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89]
    assert sum(sizes) < W
    sizes += [W - sum(sizes), 1]
    sizes += [2 * W - sum(sizes), 1]
    return sizes


def check_growth(eng, W: int):
    """After every append: the root at the new count; the roots at all earlier counts in one call
    (k = 0 and duplicates included) as they were recorded before the later appends; proofs under
    the new count and under an earlier one."""
    tid = TREE_ID
    lv = leaves(tid, 2 * W + 1)
    recorded = {0: M.Z[32]}
    with eng.create(4 * W) as tree:
        assert tree.count == 0 and tree.roots([0]) == [M.Z[32]]
        k, earlier = 0, 0
        for n in growth_sizes(W):
            tree.append(lv[k:k + n])
            k += n
            assert tree.count == k
            new = tree.roots([k])[0]
            assert new == model(tid, k).root, k
            recorded[k] = new
            counts = list(range(k + 1)) + [k, 0, earlier, earlier]
            got = tree.roots(counts)
            for c, r in zip(counts, got):
                assert r == (recorded[c] if c in recorded else model(tid, c).root), (k, c)
            for at in (k, earlier):
                check_proofs(tree, tid, at, [0, at // 2, max(at - 1, 0), at, 2 ** 31])
            earlier = k - n // 2 if n > 1 else k - n          # a count inside the last append, or its start
        assert k == 2 * W + 1


# ---------------------------------------------- one append that straddles tiles
def check_straddle_small(eng, W: int):
    """n = 3W + 5 at count W + 3, in a tree of capacity 2^17."""
    tid = TREE_ID + 1
    c0, n = W + 3, 3 * W + 5
    lv = leaves(tid, c0 + n)
    with eng.create(2 ** 17) as tree:
        tree.append(lv[:c0])
        before = tree.roots([c0])[0]
        tree.append(lv[c0:])
        k = c0 + n
        assert tree.roots([k, c0, W, 2 * W, 0]) == [model(tid, c).root for c in (k, c0, W, 2 * W)] + [M.Z[32]]
        assert before == model(tid, c0).root
        check_proofs(tree, tid, k, [0, c0 - 1, c0, 2 * W - 1, 2 * W, k - 1, k, 2 ** 31])
        check_proofs(tree, tid, c0, [0, c0 - 1, c0, k - 1])
        check_proofs(tree, tid, 2 * W + 1, [2 * W, 2 * W + 1, W])


def check_straddle_large(eng, W: int):
    """n = 2 at count W^2 - 1 -- the append crosses a tile of tiles -- then W more."""
    tid = TREE_ID + 2
    c0 = W * W - 1
    lv = leaves(tid, c0 + 2 + W)
    with eng.create(2 ** 17) as tree:
        tree.append(lv[:c0])
        tree.append(lv[c0:c0 + 2])
        assert tree.roots([c0 + 2, c0, c0 + 1]) == [model(tid, c).root for c in (c0 + 2, c0, c0 + 1)]
        tree.append(lv[c0 + 2:])
        k = c0 + 2 + W
        assert tree.count == k
        assert tree.roots([k, c0 + 1, c0]) == [model(tid, c).root for c in (k, c0 + 1, c0)]
        check_proofs(tree, tid, k, [0, c0 - 1, c0, c0 + 1, c0 + 2, k - 1, k])
        check_proofs(tree, tid, c0 + 1, [0, c0 - 1, c0, c0 + 1, k - 1])


# ------------------------------------------------------------------- capacity
def check_capacity(eng):
    """A capacity that is no power of two, filled exactly; one more leaf is rejected and changes
    nothing."""
    tid = TREE_ID + 3
    cap = 1000
    lv = leaves(tid, cap + 2)
    with eng.create(cap) as tree:
        assert tree.capacity == cap
        tree.append(lv[:600])
        tree.append(lv[600:999])
        with pytest.raises(ValueError):
            tree.append(lv[999:1001])                 # two do not fit
        assert tree.count == 999 and tree.roots([999])[0] == model(tid, 999).root
        tree.append(lv[999:1000])
        root = tree.roots([cap])[0]
        assert tree.count == cap and root == model(tid, cap).root
        with pytest.raises(ValueError):
            tree.append(lv[1000:1001])
        assert tree.count == cap and tree.roots([cap])[0] == root
        check_proofs(tree, tid, cap, [0, 511, 512, 998, 999, 1000, 1023, 1024])
        check_proofs(tree, tid, 999, [998, 999])


# --------------------------------------------------------------- small depths
def check_small_depths(eng):
    """Depth 3 with capacity 7: every count and every proof, asked as the tree grows and again
    after the last append.  Depths and capacities the header rejects."""
    tid = TREE_ID + 4
    lv = leaves(tid, 7)
    with eng.create(7, 3) as tree:
        for c in range(8):
            if c:
                tree.append(lv[c - 1:c])
            for k in range(c + 1):
                assert tree.roots([k])[0] == model(tid, k, 3).root, (c, k)
                check_proofs(tree, tid, k, range(8), 3)
        with pytest.raises(ValueError):
            tree.append(lv[:1])
    with eng.create(1, 1) as tree:
        tree.append(lv[:1])
        assert tree.roots([0, 1]) == [M.Z[1], model(tid, 1, 1).root]
        check_proofs(tree, tid, 1, [0, 1], 1)
    for capacity, depth in ((1, 0), (0, 0), (8, 3), (1, 33), (0, 32), (2 ** 32, 32)):
        with pytest.raises(ValueError):
            eng.create(capacity, depth)
    eng.create(3, 2).close()                          # 2^depth - 1 itself is fine


# ------------------------------------------------------------- rejected calls
def check_rejected(eng):
    tid = TREE_ID + 5
    lv = leaves(tid, 5)
    with eng.create(16) as tree:
        tree.append([])                               # n == 0: fine, runs nothing
        assert tree.count == 0
        tree.append(lv)
        assert tree.proofs([], 5) == ([], model(tid, 5).root)      # n_idx == 0: the root alone
        assert tree.roots([]) == []
        with pytest.raises(ValueError):
            tree.roots([6])
        with pytest.raises(ValueError):
            tree.roots([0, 5, 6, 1])
        with pytest.raises(ValueError):
            tree.proofs([0], 6)
        assert tree.count == 5 and tree.roots([5])[0] == model(tid, 5).root
