"""The cases of the SSZ list tree kept in memory, run against any engine: the
host build (test_list_tree_host.py), the library's host-pointer forms and its device forms
(test_list_tree_gpu.py).  An engine has
    create(capacity, typ) -> tree           typ: a type tuple of ssz_oracle / bls381_amd.ssz
    create_raw(capacity, item_size, prog)   prog: a uint32 array or None (packed); ValueError when rejected
    device_form                             True: updates skip an index at or above the count and
                                            run repeated indices as given; False: they reject / keep the last
    verify(leaves, proofs, depth, indices, root) -> [bool]
and a tree has
    count, depth, item_size, capacity
    append(items)                           items: a list of serialized items
    update(indices, off, length, values)    values: a list of `length`-byte strings
    root(mix) -> 32 bytes
    proofs(chunk_indices) -> ([32 * depth bytes per index], unmixed root)
    read(first, n) -> [items]
    tail() -> the bytes of the item store from the count to the capacity
    close()
each raising ValueError for arguments the engine rejects.  Expected values come from
merkle_model.Tree and ssz_oracle.hash_tree_root applied to a plain Python list that the case
mutates alongside, and from tests/golden/list_tree_history.json (the reference's
merkle_minimal.py)."""
import functools
import json
import os
import random

import pytest

import deposit_model
import merkle_model as M
import ssz_oracle as S

UINT64 = S.uint(8)
UINT8 = S.uint(1)
BYTES32 = S.Bytes(32)
PAIR16 = S.Container(("a", S.uint(8)), ("b", S.uint(8)))
# 0_beacon-chain.md Validator: 121 bytes serialized
VALIDATOR = S.Container(("pubkey", S.Bytes(48)), ("withdrawal_credentials", S.Bytes(32)),
                        ("activation_eligibility_epoch", S.uint(8)), ("activation_epoch", S.uint(8)),
                        ("exit_epoch", S.uint(8)), ("withdrawable_epoch", S.uint(8)), ("slashed", S.BOOL),
                        ("effective_balance", S.uint(8)))
FIXTURE_TYPES = {"validator": VALIDATOR, "uint64": UINT64, "bytes32": BYTES32}


def item_size(typ) -> int:
    if typ[0] == "container":
        return sum(item_size(t) for _, t in typ[1])
    return 1 if typ[0] == "bool" else typ[1]


def field_span(typ, field):
    off = 0
    for name, t in typ[1]:
        if name == field:
            return off, item_size(t)
        off += item_size(t)
    raise KeyError(field)


def deserialize(typ, b: bytes):
    k = typ[0]
    if k == "uint":
        return int.from_bytes(b, "little")
    if k == "bool":
        assert b in (b"\x00", b"\x01")
        return b == b"\x01"
    if k == "bytes":
        return b
    out, off = {}, 0
    for name, t in typ[1]:
        out[name] = deserialize(t, b[off:off + item_size(t)])
        off += item_size(t)
    return out


_TYPES = {}


@functools.lru_cache(maxsize=None)
def _item_root(type_key, item: bytes) -> bytes:
    typ = _TYPES[type_key]
    return S.hash_tree_root(typ, deserialize(typ, item))


def chunks_of(typ, items):
    if typ[0] != "container":
        return M.chunkify(b"".join(items))
    key = repr(typ)
    _TYPES[key] = typ
    return [_item_root(key, it) for it in items]


class Model:
    """hash_tree_root of the list as it stands, and the proofs of its chunks."""

    def __init__(self, typ, items):
        self.chunks = chunks_of(typ, items)
        self.count = len(items)
        self.depth = M.chunk_depth(len(self.chunks))
        self.tree = M.Tree(self.chunks, 0, self.depth)

    def root(self, mix=True) -> bytes:
        return M.mix_in_length(self.tree.root, self.count) if mix else self.tree.root

    def chunk(self, i) -> bytes:
        return self.chunks[i] if i < len(self.chunks) else M.ZERO


def rand_items(rng, typ, n):
    size = item_size(typ)
    items = [rng.randbytes(size) for _ in range(n)]
    if typ is VALIDATOR:
        items = [it[:112] + bytes([it[112] & 1]) + it[113:] for it in items]
    return items


def apply_update(items, indices, off, length, values):
    for i, v in zip(indices, values):
        assert len(v) == length
        items[i] = items[i][:off] + v + items[i][off + length:]


def split(proof: bytes):
    return [proof[i:i + 32] for i in range(0, len(proof), 32)]


def check_state(eng, tree, typ, items, proofs_of=None, read=True, model=None):
    """The tree against the model of `items`: count, depth, both roots, the whole list read back,
    zero bytes behind the count, and the proofs of `proofs_of` (chunk indices below 2^d)."""
    m = model or Model(typ, items)
    assert tree.count == len(items) and tree.depth == m.depth
    assert tree.root(True) == m.root(True) and tree.root(False) == m.root(False)
    if read:
        assert tree.read(0, len(items)) == items
        tail = tree.tail()
        assert len(tail) == (tree.capacity - len(items)) * tree.item_size and not any(tail)
    if proofs_of is not None:
        idx = sorted({i for i in proofs_of if 0 <= i < 2 ** m.depth})
        proofs, root = tree.proofs(idx)
        assert root == m.root(False)
        for i, p in zip(idx, proofs):
            assert len(p) == 32 * m.depth and split(p) == m.tree.proof(i), i
            assert deposit_model.branch_root(m.chunk(i), split(p), m.depth, i) == root, i
        if idx and m.depth:
            assert all(eng.verify([m.chunk(i) for i in idx], proofs, m.depth, idx, root))
    return m


# ---------------------------------------------------------------- 1. the fixture
@functools.lru_cache(maxsize=None)
def fixture():
    with open(os.path.join(M.ROOT, "tests", "golden", "list_tree_history.json")) as f:
        return json.load(f)


def replay(history):
    """(step, items after it) for every step of a recorded history."""
    items = []
    for st in history["steps"]:
        if st["op"] == "append":
            items += [bytes.fromhex(x) for x in st["items"]]
        else:
            apply_update(items, st["indices"], st["off"], st["len"], [bytes.fromhex(x) for x in st["values"]])
        yield st, list(items)


def check_fixture(eng, name):
    fx = fixture()[name]
    typ = FIXTURE_TYPES[name]
    assert item_size(typ) == fx["item_size"]
    with eng.create(100, typ) as tree:
        for st, items in replay(fx):
            if st["op"] == "append":
                tree.append([bytes.fromhex(x) for x in st["items"]])
            else:
                tree.update(st["indices"], st["off"], st["len"], [bytes.fromhex(x) for x in st["values"]])
            assert tree.count == len(items)
            assert tree.root(True).hex() == st["root"] and tree.root(False).hex() == st["root_unmixed"]
        assert [x.hex() for x in tree.read(0, tree.count)] == fx["final"]


# ------------------------------------------- 2. growth through depth changes
def growth_sizes(W: int):
    return [1, 1, 1, 1, 1, W - 6, 1, 1, 23, W - 23]          # counts 1 .. 5, W-1, W, W+1, W+24, 2W+1


def check_growth(eng, W: int, typ, per: int = 1):
    """Counts 0, 1, 2, 3, 4, 5, W-1, W, W+1, 2W+1 (in chunks: `per` items to a chunk) by uneven
    appends; after each the roots, the depth and the proofs of chunks 0, chunks-1, chunks, 2^d - 1."""
    rng = random.Random("growth %r" % (typ,))
    items = []
    with eng.create(per * 4 * W, typ) as tree:
        check_state(eng, tree, typ, items, [0])
        assert tree.root(False) == M.ZERO and tree.root(True) == M.mix_in_length(M.ZERO, 0)
        for n in growth_sizes(W):
            new = rand_items(rng, typ, per * n)
            tree.append(new)
            items += new
            m = Model(typ, items)
            check_state(eng, tree, typ, items, [0, len(m.chunks) - 1, len(m.chunks), 2 ** m.depth - 1], model=m)
        assert len(items) == per * (2 * W + 1)


# ------------------------------------- 3. updates inside and across tiles
def check_updates(eng, W: int, typ, per: int = 1):
    """Capacity 4W chunks, count 2W + 9: index 0; the last; W-1 and W together; every item of
    tile 1; one item in every tile; all items."""
    rng = random.Random("updates %r" % (typ,))
    n = per * (2 * W + 9)
    size = item_size(typ)
    items = rand_items(rng, typ, n)
    with eng.create(per * 4 * W, typ) as tree:
        tree.append(items)
        check_state(eng, tree, typ, items)
        for idx in ([0], [n - 1], [per * W - 1, per * W], list(range(per * W, 2 * per * W)),
                    [5, per * W + 5, 2 * per * W + 5], list(range(n))):
            vals = rand_items(rng, typ, len(idx))
            tree.update(idx, 0, size, vals)
            apply_update(items, idx, 0, size, vals)
            check_state(eng, tree, typ, items, [idx[0] // per, idx[-1] // per])


# -------------------------------------------------------- 4. three passes
def check_three_passes(eng, W: int, typ, per: int = 1):
    """A chunk capacity of W W + W: rows up to level 17, three passes.  (`per` items to a chunk:
    a packed uint64 list needs 4 (W W + W) items for that height, so the issue's counts are taken
    in chunks.)  Append to one item short of W W chunks, append 2 -- the append crosses a tile of
    tiles; update the first item and the two around the crossing; append W - 1 chunks more;
    update an item appended before the crossing."""
    rng = random.Random("three passes %r" % (typ,))
    size = item_size(typ)
    items = rand_items(rng, typ, per * W * W - 1)
    with eng.create(per * (W * W + W), typ) as tree:
        tree.append(items)
        check_state(eng, tree, typ, items, read=False)
        new = rand_items(rng, typ, 2)
        tree.append(new)
        items += new
        check_state(eng, tree, typ, items, read=False)
        idx = [0, per * W * W - 1, per * W * W]
        vals = rand_items(rng, typ, 3)
        tree.update(idx, 0, size, vals)
        apply_update(items, idx, 0, size, vals)
        check_state(eng, tree, typ, items, [0, W * W - 1, W * W], read=False)
        new = rand_items(rng, typ, per * (W - 1))
        tree.append(new)
        items += new
        check_state(eng, tree, typ, items, read=False)
        idx = [per * (W * W - W) + 3]
        vals = rand_items(rng, typ, 1)
        tree.update(idx, 0, size, vals)
        apply_update(items, idx, 0, size, vals)
        check_state(eng, tree, typ, items, [W * W - W, W * W + W - 1], read=True)


# ------------------------------------------------ 5. packed partial chunks
def check_packed_partial(eng):
    rng = random.Random("partial")
    items = []
    with eng.create(40, UINT64) as tree:
        for c in range(1, 10):                                   # counts 1 .. 9, one item at a time
            new = rand_items(rng, UINT64, 1)
            tree.append(new)
            items += new
            check_state(eng, tree, UINT64, items, [0, (c - 1) // 4])
        for idx in ([8], [7], [3, 8]):                           # the partial last chunk; the chunk before it
            vals = rand_items(rng, UINT64, len(idx))
            tree.update(idx, 0, 8, vals)
            apply_update(items, idx, 0, 8, vals)
            check_state(eng, tree, UINT64, items, [0, 1, 2])
        tree.update([5], 0, 8, [b"\x11" * 8])                    # chunk 1, then an append into partial chunk 2
        apply_update(items, [5], 0, 8, [b"\x11" * 8])
        new = rand_items(rng, UINT64, 2)
        tree.append(new)
        items += new
        check_state(eng, tree, UINT64, items, [0, 1, 2, 3])
        tree.update([10], 3, 2, [b"\xAB\xCD"])                   # two bytes inside an item
        apply_update(items, [10], 3, 2, [b"\xAB\xCD"])
        check_state(eng, tree, UINT64, items, [2])
    items = rand_items(rng, UINT8, 31)
    with eng.create(70, UINT8) as tree:                          # item_size 1: 31, 32, 33 items
        tree.append(items)
        for _ in range(2):
            check_state(eng, tree, UINT8, items, [0, 1])
            new = rand_items(rng, UINT8, 1)
            tree.append(new)
            items += new
        assert len(items) == 33
        check_state(eng, tree, UINT8, items, [0, 1])
        tree.update([32, 31], 0, 1, [b"\x7f", b"\x80"])
        apply_update(items, [32, 31], 0, 1, [b"\x7f", b"\x80"])
        check_state(eng, tree, UINT8, items, [0, 1])
    items = rand_items(rng, BYTES32, 3)
    with eng.create(5, BYTES32) as tree:                         # the store is row 0
        tree.append(items)
        check_state(eng, tree, BYTES32, items, [0, 1, 2, 3])
        tree.update([1], 30, 2, [b"\x01\x02"])
        apply_update(items, [1], 30, 2, [b"\x01\x02"])
        check_state(eng, tree, BYTES32, items, [0, 1, 2, 3])
        assert tree.read(1, 2) == items[1:3] and tree.read(3, 0) == []


# ------------------------------------- 6. field updates on Validator records
VALIDATOR_COUNT = 300


def validator_field_steps(rng, n):
    """(field, indices, values as bytes) of the state transition's writes, scattered."""
    return [("effective_balance", sorted(rng.sample(range(n), 7)), [rng.randbytes(8) for _ in range(7)]),
            ("slashed", [3, n - 1, 255, 256], [b"\x01", b"\x01", b"\x00", b"\x01"]),
            ("exit_epoch", sorted(rng.sample(range(n), 5)), [rng.randrange(2 ** 20).to_bytes(8, "little") for _ in range(5)]),
            ("effective_balance", [0], [(32 * 10 ** 9).to_bytes(8, "little")])]


def check_validator_fields(eng, tree=None):
    """effective_balance (offset 113, unaligned), slashed (112, one byte) and exit_epoch (96) of
    scattered records; untouched records read back byte-equal.  Returns the records."""
    assert [field_span(VALIDATOR, f) for f in ("effective_balance", "slashed", "exit_epoch")] == [(113, 8), (112, 1), (96, 8)]
    assert item_size(VALIDATOR) == 121
    rng = random.Random("validator fields")
    n = VALIDATOR_COUNT
    items = rand_items(rng, VALIDATOR, n)
    own = tree is None
    tree = tree or eng.create(2 * n, VALIDATOR)
    try:
        tree.append(items[:100])
        tree.append(items[100:])
        check_state(eng, tree, VALIDATOR, items)
        for field, idx, vals in validator_field_steps(rng, n):
            off, length = field_span(VALIDATOR, field)
            before = list(items)
            tree.update(idx, off, length, vals)
            apply_update(items, idx, off, length, vals)
            assert all(items[i] == before[i] for i in range(n) if i not in idx)
            check_state(eng, tree, VALIDATOR, items, [idx[0], idx[-1]])
    finally:
        if own:
            tree.close()
    return items


# --------------------------------------------------- 8. repeated indices
def check_repeated(eng, W: int):
    rng = random.Random("repeated")
    typ = PAIR16
    items = rand_items(rng, typ, W + 5)
    with eng.create(2 * W, typ) as tree:
        tree.append(items)
        a, b, c = rand_items(rng, typ, 3)
        if not eng.device_form:
            tree.update([7, W, 7], 0, 16, [a, b, c])             # applied in order: the last wins
            apply_update(items, [7, W, 7], 0, 16, [a, b, c])
            check_state(eng, tree, typ, items, [7, W])
            root = tree.root(True)
            with pytest.raises(ValueError):
                tree.update([0, W + 5], 0, 16, [a, b])           # an index at the count: nothing changes
            with pytest.raises(ValueError):
                tree.update([2 ** 32 - 1], 0, 16, [a])
            check_state(eng, tree, typ, items)
            assert tree.root(True) == root
            return
        tree.update([7, W, 7, W], 0, 16, [a, b, a, b])           # equal values
        apply_update(items, [7, W], 0, 16, [a, b])
        check_state(eng, tree, typ, items, [7, W])
        tree.update([9, 9, W + 1, 9], 0, 16, [a, b, c, c])       # different values: one of them, byte by byte
        got = tree.read(0, len(items))
        assert all(got[9][k] in (a[k], b[k], c[k]) for k in range(16)) and got[W + 1] == c
        assert [g for i, g in enumerate(got) if i not in (9, W + 1)] == [x for i, x in enumerate(items) if i not in (9, W + 1)]
        items = got
        check_state(eng, tree, typ, items, [9, W + 1])           # the tree is the tree of what the store holds
        root = tree.root(True)
        tree.update([W + 5, 2 ** 32 - 1, W + 6], 0, 16, [a, b, c])     # at or above the count: skipped
        check_state(eng, tree, typ, items)
        assert tree.root(True) == root and tree.tail()[:32] == bytes(32)
        tree.update([W + 5, 3], 4, 2, [b"\x01\x02", b"\x03\x04"])      # a skipped index beside a real one
        apply_update(items, [3], 4, 2, [b"\x03\x04"])
        check_state(eng, tree, typ, items, [3])


# ------------------------------------------------------ 10. rejected calls
def check_rejected(eng, good_prog):
    """Every rejection the engines share, with the count and the root unchanged afterwards."""
    for capacity, size, prog in ((0, 8, None), (2 ** 31, 8, None), (4, 0, None), (4, 3, None), (4, 64, None),
                                 (4, 121, None), (4, 0, good_prog), (4, 15, good_prog)):      # the program reads 16 bytes
        with pytest.raises(ValueError):
            eng.create_raw(capacity, size, prog)
    eng.create_raw(4, 16, good_prog).close()
    eng.create_raw(4, 17, good_prog).close()
    rng = random.Random("rejected")
    for typ in (PAIR16, UINT64):
        size = item_size(typ)
        items = rand_items(rng, typ, 5)
        with eng.create(6, typ) as tree:
            tree.append([])                                      # n == 0: fine, runs nothing
            tree.update([], 0, size, [])
            assert tree.count == 0 and tree.root(False) == M.ZERO
            tree.append(items)
            root = tree.root(True)
            with pytest.raises(ValueError):
                tree.append(rand_items(rng, typ, 2))             # two do not fit
            tree.update([0], 0, 0, [b""])                        # len == 0: fine, runs nothing
            tree.update([], 0, size, [])
            for off, length in ((size, 1), (0, size + 1), (size + 1, 0), (1, size)):
                with pytest.raises(ValueError):
                    tree.update([0], off, length, [bytes(length)])
            with pytest.raises(ValueError):
                tree.read(0, 6)
            with pytest.raises(ValueError):
                tree.read(6, 0)
            assert tree.proofs([]) == ([], Model(typ, items).root(False))
            assert tree.count == 5 and tree.root(True) == root == Model(typ, items).root(True)
            assert tree.read(0, 5) == items
            tree.append(rand_items(rng, typ, 1))                 # filled exactly
            with pytest.raises(ValueError):
                tree.append(rand_items(rng, typ, 1))
            assert tree.count == 6
