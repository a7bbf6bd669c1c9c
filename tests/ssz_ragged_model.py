"""Plain-Python model of the roots of variable-size SSZ containers: serialization,
hash_tree_root from a value, and hash_tree_root from serialized bytes with the validity rules an
untrusted item must keep.  Pinned to tests/golden/ssz_ragged.json (the reference's own ssz_impl
lines, see tests/golden/make_ssz_ragged_vectors.py) by tests/test_ssz_ragged_host.py; the host
build and the kernels are then compared with this model.

Types are the plain tuples of bls381_amd.ssz.  Values are Python ints, bools, bytes, lists and dicts.
The fixture gives values by a seed rule (``Stream``, ``value_for``) so that it stays small.
"""
import hashlib
import itertools

from bls381_amd import ssz as S


def H(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


ZERO = [b"\x00" * 32]
for _ in range(40):
    ZERO.append(H(ZERO[-1] + ZERO[-1]))


def merkleize(chunks) -> bytes:
    """merkle_minimal.py merkleize_chunks: zero chunks up to a power of two; no chunks give the zero chunk."""
    layer = list(chunks)
    if not layer:
        return ZERO[0]
    depth = (len(layer) - 1).bit_length()
    for h in range(depth):
        if len(layer) % 2:
            layer.append(ZERO[h])
        layer = [H(layer[i] + layer[i + 1]) for i in range(0, len(layer), 2)]
    return layer[0]


def mix_in_length(root: bytes, n: int) -> bytes:
    return H(root + n.to_bytes(32, "little"))


def chunkify(b: bytes):
    b = b + b"\x00" * (-len(b) % 32)
    return [b[i:i + 32] for i in range(0, len(b), 32)]


def is_basic(t) -> bool:
    return t[0] in ("uint", "bool")


def is_fixed(t) -> bool:
    k = t[0]
    if k == "list":
        return False
    if k == "vector":
        return is_fixed(t[1])
    if k == "container":
        return all(is_fixed(ft) for _, ft in t[1])
    return True


def size(t) -> int:
    k = t[0]
    if k == "uint":
        return t[1]
    if k == "bool":
        return 1
    if k == "bytes":
        return t[1]
    if k == "vector":
        return t[2] * size(t[1])
    return sum(size(ft) for _, ft in t[1])


def fixed_part(t) -> int:
    return sum(size(ft) if is_fixed(ft) else 4 for _, ft in t[1])


def _series(types, values) -> bytes:
    parts = [(is_fixed(t), serialize(t, v)) for t, v in zip(types, values)]
    off = sum(len(p) if f else 4 for f, p in parts)
    head, tail = [], []
    for f, p in parts:
        if f:
            head.append(p)
        else:
            head.append(off.to_bytes(4, "little"))
            tail.append(p)
            off += len(p)
    return b"".join(head + tail)


def serialize(t, v) -> bytes:
    k = t[0]
    if k == "uint":
        return int(v).to_bytes(t[1], "little")
    if k == "bool":
        return b"\x01" if v else b"\x00"
    if k == "bytes":
        assert len(v) == t[1]
        return bytes(v)
    if k in ("list", "vector"):
        if isinstance(v, bytes):
            return v
        return _series([t[1]] * len(v), v)
    return _series([ft for _, ft in t[1]], [v[name] for name, _ in t[1]])


def root(t, v) -> bytes:
    """hash_tree_root of a value (ssz_impl.py:143-155)."""
    k = t[0]
    if is_basic(t) or k == "bytes":
        return merkleize(chunkify(serialize(t, v)))
    if k in ("list", "vector"):
        if is_basic(t[1]):
            leaves = chunkify(serialize(t, v))
        else:
            leaves = [root(t[1], x) for x in v]
        r = merkleize(leaves)
        return mix_in_length(r, len(v)) if k == "list" else r
    return merkleize([root(ft, v[name]) for name, ft in t[1]])


def signing_root(t, v) -> bytes:
    return merkleize([root(ft, v[name]) for name, ft in t[1][:-1]])


class Malformed(Exception):
    pass


def _root_fixed_bytes(t, b: bytes) -> bytes:
    k = t[0]
    if is_basic(t) or k == "bytes" or (k == "vector" and is_basic(t[1])):
        return merkleize(chunkify(b))
    if k == "vector":
        n = size(t[1])
        return merkleize([_root_fixed_bytes(t[1], b[i * n:(i + 1) * n]) for i in range(t[2])])
    out, off = [], 0
    for _, ft in t[1]:
        out.append(_root_fixed_bytes(ft, b[off:off + size(ft)]))
        off += size(ft)
    return merkleize(out)


def _root_scope(t, b: bytes) -> bytes:
    """The root of the variable-size container serialized in b, the rules checked first."""
    fixed = fixed_part(t)
    if len(b) < fixed:
        raise Malformed("the scope is shorter than its fixed part")
    pos, off = [], 0
    for _, ft in t[1]:
        pos.append(off)
        off += size(ft) if is_fixed(ft) else 4
    var = [i for i, (_, ft) in enumerate(t[1]) if not is_fixed(ft)]
    offs = [int.from_bytes(b[pos[i]:pos[i] + 4], "little") for i in var]
    if offs and offs[0] != fixed:
        raise Malformed("the first offset is not the fixed part's size")
    if any(x > y for x, y in zip(offs, offs[1:])):
        raise Malformed("offsets decrease")
    if offs and offs[-1] > len(b):
        raise Malformed("the last offset is past the scope")
    ends = dict(zip(var, offs[1:] + [len(b)]))
    begins = dict(zip(var, offs))
    out = []
    for i, (_, ft) in enumerate(t[1]):
        if is_fixed(ft):
            out.append(_root_fixed_bytes(ft, b[pos[i]:pos[i] + size(ft)]))
            continue
        seg = b[begins[i]:ends[i]]
        if ft[0] == "list" and is_basic(ft[1]):
            if len(seg) % size(ft[1]):
                raise Malformed("a field's length is not a multiple of its element size")
            out.append(mix_in_length(merkleize(chunkify(seg)), len(seg) // size(ft[1])))
        elif ft[0] == "container":
            out.append(_root_scope(ft, seg))
        else:
            raise ValueError("not a ragged type")
    return merkleize(out)


def root_from_bytes(t, item: bytes):
    """(status, root) as the engine gives them: (0, hash_tree_root) for a well-formed item,
    (1, 32 zero bytes) for one that breaks a rule."""
    try:
        return 0, _root_scope(t, bytes(item))
    except Malformed:
        return 1, b"\x00" * 32


def list_root(t, items) -> bytes:
    """hash_tree_root of List[t] from the serialized items."""
    roots = []
    for x in items:
        st, r = root_from_bytes(t, x)
        if st:
            raise Malformed("item")
        roots.append(r)
    return mix_in_length(merkleize(roots), len(roots))


# ---- the fixture's seed rule
class Stream:
    """Bytes from SHA-256(seed || counter as 8 bytes little-endian), counter 0, 1, ...; zero=True: zero bytes."""

    def __init__(self, seed: str, zero: bool = False):
        self.seed, self.ctr, self.buf, self.zero = seed.encode(), 0, b"", zero

    def bytes(self, n: int) -> bytes:
        if self.zero:
            return b"\x00" * n
        while len(self.buf) < n:
            self.buf += H(self.seed + self.ctr.to_bytes(8, "little"))
            self.ctr += 1
        out, self.buf = self.buf[:n], self.buf[n:]
        return out


def value_for(t, st: Stream, sizes):
    """A value of type t: fixed parts from the stream, each list's length the next of `sizes`
    (an iterator), fields and elements in order."""
    k = t[0]
    if k == "uint":
        return int.from_bytes(st.bytes(t[1]), "little")
    if k == "bool":
        return bool(st.bytes(1)[0] & 1)
    if k == "bytes":
        return st.bytes(t[1])
    if k == "vector":
        return [value_for(t[1], st, sizes) for _ in range(t[2])]
    if k == "list":
        n = next(sizes)
        if t[1] == S.uint(1):
            return st.bytes(n)
        return [value_for(t[1], st, sizes) for _ in range(n)]
    return {name: value_for(ft, st, sizes) for name, ft in t[1]}


def case_value(case):
    """The value of a fixture case {"type", "seed", "sizes", "zero"}."""
    return value_for(getattr(S, case["type"]), Stream(case["seed"], case.get("zero", False)),
                     itertools.cycle(case["sizes"]))


def list_case_values(case):
    """The elements of a fixture list case {"type", "n", "seed", "sizes"}: element i takes the seed
    "<seed>:<i>" and the sizes rotated left by i, so neighbours differ in length."""
    t, sz = getattr(S, case["type"]), case["sizes"]
    return [value_for(t, Stream("%s:%d" % (case["seed"], i)), itertools.cycle(sz[i % len(sz):] + sz[:i % len(sz)]))
            for i in range(case["n"])]


# ---- malformed items: each validity rule broken in turn
def offset_positions(t):
    """Positions of the offset words in the fixed part of container t."""
    pos, off = [], 0
    for _, ft in t[1]:
        if not is_fixed(ft):
            pos.append(off)
        off += size(ft) if is_fixed(ft) else 4
    return pos


def _with_word(b: bytes, pos: int, value: int) -> bytes:
    return b[:pos] + (value & 0xFFFFFFFF).to_bytes(4, "little") + b[pos + 4:]


def malformed(t, ser: bytes):
    """[(label, item)]: a well-formed item of container t with one rule broken at a time (and, for
    a container with nested scopes, the same inside the first nested scope)."""
    fixed, pos = fixed_part(t), offset_positions(t)
    first = int.from_bytes(ser[pos[0]:pos[0] + 4], "little")
    out = [("empty item", b""),
           ("scope shorter than its fixed part", ser[:fixed - 1]),
           ("first offset above the fixed part", _with_word(ser, pos[0], first + 1)),
           ("first offset below the fixed part", _with_word(ser, pos[0], first - 1)),
           ("last offset past the scope", _with_word(ser, pos[-1], len(ser) + 1)),
           ("last offset 2^32 - 1", _with_word(ser, pos[-1], 0xFFFFFFFF))]
    if len(pos) > 1:
        out.append(("offsets decrease", _with_word(ser, pos[1], first - 1)))
        out.append(("second offset past the scope", _with_word(ser, pos[1], len(ser) + 4)))
    last = [ft for _, ft in t[1] if not is_fixed(ft)][-1]
    if last[0] == "list" and size(last[1]) > 1:
        out.append(("field length no multiple of the element size", ser + b"\x00"))
        out.append(("field one byte short", ser[:-1] if len(ser) > first else ser + b"\x00\x00\x00"))
    nested = [ft for _, ft in t[1] if not is_fixed(ft) and ft[0] == "container"]
    if nested:
        inner = nested[0]
        ipos = offset_positions(inner)
        ifirst = int.from_bytes(ser[first + ipos[0]:first + ipos[0] + 4], "little")
        out.append(("nested scope shorter than its fixed part", _with_word(ser, pos[1], first + fixed_part(inner) - 1)))
        out.append(("nested first offset", _with_word(ser, first + ipos[0], ifirst + 8)))
        out.append(("nested offsets decrease", _with_word(ser, first + ipos[1], ifirst - 8)))
        out.append(("nested last offset past its scope", _with_word(ser, first + ipos[-1], len(ser))))
    for label, item in out:
        assert root_from_bytes(t, item)[0] == 1, label
    return out
