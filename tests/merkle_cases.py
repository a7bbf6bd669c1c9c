"""The cases of the Merkle tree primitive, run against any engine: the host build
(test_merkle_tree_host.py), the library's host-pointer forms and its device forms
(test_merkle_tree_gpu.py).  An engine has
    root(leaves, depth, first=0, length=None) -> 32 bytes
    proofs(leaves, depth, indices, first=0) -> ([32 * depth bytes per index], root)
and raises ValueError for arguments the engine rejects.  Expected values come from
tests/golden/merkle_trees.json and from merkle_model.py; a model tree is built once per case
and shared between the engines."""
import functools
import hashlib

import pytest

import deposit_model
import merkle_model as M


@functools.lru_cache(maxsize=None)
def leaves(tree_id: int, n: int):
    return tuple(M.leaves_of(tree_id, n))


@functools.lru_cache(maxsize=None)
def model(tree_id: int, n: int, first: int, depth: int) -> M.Tree:
    return M.Tree(leaves(tree_id, n), first, depth)


def sha(parts) -> str:
    return hashlib.sha256(b"".join(parts)).hexdigest()


def split(proof: bytes):
    return [proof[i:i + 32] for i in range(0, len(proof), 32)]


# ---------------------------------------------------------------- the fixture
def check_fixture_tree(eng, t):
    """One "trees" entry: root, every proof by digest, three proofs outside the window in full,
    merkleize_chunks."""
    n, lv = t["n"], leaves(t["id"], t["n"])
    assert eng.root(lv, 32).hex() == t["root"]
    proofs, root = eng.proofs(lv, 32, range(n))
    assert root.hex() == t["root"] and sha(proofs) == t["proofs_sha256"]
    outside = [n, n + 1, 2 ** 31]
    proofs, root = eng.proofs(lv, 32, outside)
    assert root.hex() == t["root"]
    for i, p in zip(outside, proofs):
        assert [s.hex() for s in split(p)] == t["proofs"][str(i)], (n, i)
    assert eng.root(lv, M.chunk_depth(n)).hex() == t["chunks_root"]


def check_fixture_large(eng, t):
    lv = leaves(t["id"], t["n"])
    assert eng.root(lv, 32).hex() == t["root"]
    assert eng.root(lv, M.chunk_depth(t["n"])).hex() == t["chunks_root"]


def check_fixture_window(eng, t):
    first, n = t["first"], t["n"]
    lv = leaves(t["id"], n)
    assert eng.root(lv, 32, first).hex() == t["root"]
    wanted = [first, first + n - 1, 0]
    proofs, root = eng.proofs(lv, 32, wanted, first)
    assert root.hex() == t["root"]
    for i, p in zip(wanted, proofs):
        assert [s.hex() for s in split(p)] == t["proofs"][str(i)], (first, n, i)


def check_fixture_empty(eng, fx):
    assert eng.root([], 0).hex() == fx["chunks0"] == M.ZERO.hex()


# ------------------------------------------------------------ tile boundaries
TILE_ID = 100          # tree ids of the cases below (the fixture's are 0 .. 21)


def tile_sizes(W: int):
    """n around one tile and around a tile of tiles; sizes above 2^20 are left out."""
    sizes = [W - 1, W, W + 1, W * W - 1, W * W, W * W + 1]
    return [n for n in sizes if n <= 2 ** 20], [n for n in sizes if n > 2 ** 20]


def check_tile_size(eng, n: int):
    """first = 0, depth 32 and the merkleize depth: roots, and proofs at the window's edges, one
    tile in, outside it and far away."""
    lv = leaves(TILE_ID, n)
    for depth in (32, M.chunk_depth(n)):
        m = model(TILE_ID, n, 0, depth)
        assert eng.root(lv, depth) == m.root, (n, depth)
        idx = sorted({i for i in (0, 1, n // 2, n - 1, n, n + 1, 2 ** 31) if i < 2 ** depth})
        proofs, root = eng.proofs(lv, depth, idx)
        assert root == m.root
        for i, p in zip(idx, proofs):
            assert split(p) == m.proof(i), (n, depth, i)


def tile_windows(W: int):
    return [(W - 1, 2), (W, 1), (2 ** 32 - 3, 3)]


def check_tile_window(eng, first: int, n: int):
    """A window that straddles a tile, one that starts one, and the last three leaves of the
    deposit tree: the root, and the proofs of the window's ends, its neighbours and leaf 0."""
    lv = leaves(TILE_ID + 1, n)
    m = model(TILE_ID + 1, n, first, 32)
    assert eng.root(lv, 32, first) == m.root
    idx = sorted({i for i in (0, first - 1, first, first + n - 1, first + n) if 0 <= i < 2 ** 32})
    proofs, root = eng.proofs(lv, 32, idx, first)
    assert root == m.root
    for i, p in zip(idx, proofs):
        assert split(p) == m.proof(i), (first, n, i)
    if first == 2 ** 32 - 3:
        for k in range(n):          # each proof folds to the root by the spec's verify_merkle_branch
            i = idx.index(first + k) if first + k in idx else None
            p = proofs[i] if i is not None else eng.proofs(lv, 32, [first + k], first)[0][0]
            assert deposit_model.branch_root(lv[k], split(p), 32, first + k) == m.root


# ---------------------------------------------------------------- depth edges
def check_depth_edges(eng, W: int):
    one = leaves(TILE_ID + 2, 1)
    assert eng.root([], 0) == M.Z[0]
    assert eng.root([], 32) == M.Z[32]
    assert eng.root(one, 0) == one[0]
    assert eng.proofs(one, 0, [0]) == ([b""], one[0])          # depth 0: nothing written
    assert eng.proofs([], 32, [0, 5]) == ([b"".join(M.Z[:32])] * 2, M.Z[32])
    logw = W.bit_length() - 1
    for n, depth in ((3, 2), (W, logw), (5, 64)):
        lv = leaves(TILE_ID + 2, n)
        m = model(TILE_ID + 2, n, 0, depth)
        assert eng.root(lv, depth) == m.root, (n, depth)
        idx = [0, n - 1] + ([2 ** 63 + 1] if depth == 64 else [])
        proofs, root = eng.proofs(lv, depth, idx)
        assert root == m.root and [split(p) for p in proofs] == [m.proof(i) for i in idx]
    five = leaves(TILE_ID + 2, 5)
    high = 2 ** 64 - 6                  # a window that ends at the last leaf of a depth-64 tree but one
    m = model(TILE_ID + 2, 5, high, 64)
    assert eng.root(five, 64, high) == m.root
    assert [split(p) for p in eng.proofs(five, 64, [high, 0], high)[0]] == [m.proof(high), m.proof(0)]


def check_rejected(eng):
    nine = leaves(TILE_ID + 2, 9)
    for lv, depth, first in ((nine, 3, 0),                 # n = 2^d + 1
                             (nine[:2], 3, 7),             # first + n > 2^d
                             (nine[:1], 65, 0),            # d = 65
                             (nine[:2], 64, 2 ** 64 - 1),  # first + n overflows
                             (nine[:2], 0, 0)):
        with pytest.raises(ValueError):
            eng.root(lv, depth, first)
        with pytest.raises(ValueError):
            eng.proofs(lv, depth, [0], first)
    assert eng.root(nine[:8], 3) == model(TILE_ID + 2, 8, 0, 3).root      # the full tree beside it is fine
    assert eng.root(nine[:1], 3, 7) == model(TILE_ID + 2, 1, 7, 3).root


# ----------------------------------------------------------------- length mix
def check_length_mix(eng):
    """hash_tree_root of List[uint64] with 5 elements: 2 chunks, length 5 -- the length is not the
    leaf count -- then lengths 0 and 2^64 - 1."""
    values = [3, 2 ** 64 - 1, 0, 7, 2 ** 40]
    want = M.hash_tree_root(M.List(("uint", 8)), values)
    chunks = M.chunkify(M.pack(values, ("uint", 8)))
    assert len(chunks) == 2
    assert eng.root(chunks, 1, 0, 5) == want == M.mix_in_length(M.merkleize_chunks(chunks), 5)
    assert eng.root(chunks, 1, 0, 2) != want
    for length in (0, 2 ** 64 - 1):
        assert eng.root(chunks, 1, 0, length) == M.mix_in_length(M.merkleize_chunks(chunks), length)
        assert eng.root([], 0, 0, length) == M.mix_in_length(M.ZERO, length)
    lv = leaves(TILE_ID + 3, 300)
    assert eng.root(lv, 32, 5, 300) == M.mix_in_length(model(TILE_ID + 3, 300, 5, 32).root, 300)
