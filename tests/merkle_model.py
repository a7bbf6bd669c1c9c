"""Pure-Python restatements (hashlib only) used by test_merkle_tree_host.py and
test_merkle_tree_gpu.py:

* the windowed tree primitive, tree(leaves[0..n), first, depth), as a list of levels: level h
  holds the real nodes first >> h .. (first+n-1) >> h, every other node of the level is Z[h];
* ssz_impl.py:110-163 of the reference (pack, chunkify, mix_in_length, hash_tree_root,
  signing_root) over the type tuples of bls381_amd/ssz.py -- uint, bool, BytesN, bytes, Vector,
  List, Container -- because the reference's ssz_typing.py does not import on this Python.

tests/golden/merkle_trees.json (make_merkle_tree_vectors.py, from the reference's
merkle_minimal.py) pins the primitive; test_merkle_tree_host.py checks this model against it.
"""
import hashlib
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZERO = b"\x00" * 32


def h(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


Z = [ZERO]
for _ in range(64):
    Z.append(h(Z[-1] + Z[-1]))


def leaves_of(tree_id: int, n: int, start: int = 0):
    """The fixture's leaves: sha256(b"leaf" + id (4 B LE) + i (8 B LE))."""
    return [h(b"leaf" + tree_id.to_bytes(4, "little") + i.to_bytes(8, "little")) for i in range(start, start + n)]


def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "merkle_trees.json")) as f:
        return json.load(f)


class Tree:
    """levels[h] = (base, [nodes]): the real nodes of level h, h = 0 .. depth."""

    def __init__(self, leaves, first: int, depth: int):
        n = len(leaves)
        assert 0 <= depth <= 64 and first + n <= 2 ** depth
        self.first, self.depth, self.n = first, depth, n
        self.levels = [(first, list(leaves))]
        for lvl in range(depth):
            base, nodes = self.levels[-1]
            if not nodes:
                self.levels.append((base >> 1, []))
                continue

            def node(j, base=base, nodes=nodes, lvl=lvl):
                return nodes[j - base] if base <= j < base + len(nodes) else Z[lvl]
            lo, hi = base >> 1, (base + len(nodes) - 1) >> 1
            self.levels.append((lo, [h(node(2 * j) + node(2 * j + 1)) for j in range(lo, hi + 1)]))
        top = self.levels[depth][1]
        assert len(top) <= 1
        self.root = top[0] if top else Z[depth]

    def node(self, lvl: int, j: int) -> bytes:
        base, nodes = self.levels[lvl]
        return nodes[j - base] if base <= j < base + len(nodes) else Z[lvl]

    def proof(self, i: int):
        return [self.node(lvl, (i >> lvl) ^ 1) for lvl in range(self.depth)]


def merkle_root(leaves, depth: int, first: int = 0, length=None) -> bytes:
    root = Tree(leaves, first, depth).root
    return root if length is None else mix_in_length(root, length)


def chunk_depth(n: int) -> int:
    return 0 if n <= 1 else (n - 1).bit_length()


def merkleize_chunks(chunks) -> bytes:
    return merkle_root(chunks, chunk_depth(len(chunks)))


# ------------------------------------------------------------ ssz_impl.py:110-163
def List(elem):
    return ("list", elem)


BYTES = ("list", ("uint", 1))      # `bytes`: a list of bytes


def is_basic(typ) -> bool:
    return typ[0] in ("uint", "bool")


def serialize_basic(typ, v) -> bytes:
    if typ[0] == "uint":
        return int(v).to_bytes(typ[1], "little")
    return b"\x01" if v else b"\x00"


def pack(values, subtype) -> bytes:
    if isinstance(values, (bytes, bytearray)):
        return bytes(values)
    return b"".join(serialize_basic(subtype, v) for v in values)


def chunkify(b: bytes):
    b = b + b"\x00" * (-len(b) % 32)
    return [b[i:i + 32] for i in range(0, len(b), 32)]


def mix_in_length(root: bytes, length: int) -> bytes:
    return h(root + int(length).to_bytes(32, "little"))


def elem_type(typ):
    return ("uint", 1) if typ[0] == "bytes" else typ[1]


def hash_tree_root(typ, v) -> bytes:
    k = typ[0]
    series = k in ("list", "vector", "bytes")
    if is_basic(typ):
        leaves = chunkify(serialize_basic(typ, v))
    elif series and is_basic(elem_type(typ)):
        leaves = chunkify(pack(v, elem_type(typ)))
    elif series:
        leaves = [hash_tree_root(typ[1], x) for x in v]
    else:
        leaves = [hash_tree_root(t, v[name]) for name, t in typ[1]]
    if k == "list":
        return mix_in_length(merkleize_chunks(leaves), len(v))
    return merkleize_chunks(leaves)


def signing_root(typ, v) -> bytes:
    assert typ[0] == "container"
    leaves = [hash_tree_root(t, v[name]) for name, t in typ[1][:-1]]
    return merkleize_chunks(chunkify(b"".join(leaves)))
