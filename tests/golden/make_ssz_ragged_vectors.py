"""Roots of variable-size SSZ containers by the reference's own ssz_impl lines.

The reference's utils/ssz/ssz_typing.py does not import on this Python (3.10: TypeError
"issubclass() arg 1 must be a class" at import), so utils/ssz/ssz_impl.py cannot be imported.  As
tests/golden/make_spec_text_vectors.py does for the BLS spec text, this script reads ssz_impl.py
at generation time and executes its text with the two import statements at its top replaced: the
names of ``ssz_typing`` come from the minimal stand-in type layer below (uintN, bool, bytes, BytesN,
List, Vector, Container), and ``merkleize_chunks`` / ``hash`` from the reference's
utils/merkle_minimal.py, imported as it is.  ``serialize``, ``hash_tree_root`` and ``signing_root``
are then the reference's own lines.  No reference text is written anywhere.

Values follow the seed rule of tests/ssz_ragged_model.py (``Stream``, ``value_for``): the fixture
records type, seed and list sizes, the length and SHA-256 of the reference's serialization, and
the reference's root.  The model is checked against each as it is written.

Output: tests/golden/ssz_ragged.json.  Tests read only the JSON.

Run where the reference is present:
    python tests/golden/make_ssz_ragged_vectors.py
"""
import hashlib
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("BLS381_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", "..", "consensus-specs_amd"))
import ssz_ragged_model as M  # noqa: E402
from bls381_amd import ssz as S  # noqa: E402  (the types: plain tuples)

IMPL = os.path.join(REF, "test_libs", "pyspec", "eth2spec", "utils", "ssz", "ssz_impl.py")


# ---- the stand-in for ssz_typing: just what ssz_impl.py asks of a type
class uint(int):
    byte_len = 0


def _uint(n):
    return type("uint%d" % (8 * n), (uint,), {"byte_len": n})


class SeriesType:
    def __init__(self, elem, length=None):
        self.elem, self.length = elem, length


class BytesN(bytes):
    pass


class Container:
    fields = ()

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @classmethod
    def get_field_types(cls):
        return [t for _, t in cls.fields]

    def get_field_values(self):
        return [getattr(self, name) for name, _ in self.fields]

    def get_typed_values(self):
        return list(zip(self.get_field_values(), self.get_field_types()))


def is_uint_type(t):
    return isinstance(t, type) and issubclass(t, uint)


def is_bool_type(t):
    return t is bool


def is_container_type(t):
    return isinstance(t, type) and issubclass(t, Container)


def is_list_kind(t):
    return t is bytes or (isinstance(t, SeriesType) and t.length is None)


def is_vector_kind(t):
    return (isinstance(t, type) and issubclass(t, BytesN)) or (isinstance(t, SeriesType) and t.length is not None)


BYTE = _uint(1)


def read_elem_type(t):
    return t.elem if isinstance(t, SeriesType) else BYTE


def infer_input_type(fn):
    def helper(obj, typ=None, **kw):
        assert typ is not None, "the generator always names the type"
        return fn(obj, typ=typ, **kw)
    return helper


STAND_IN = {
    "is_uint_type": is_uint_type, "is_bool_type": is_bool_type, "is_container_type": is_container_type,
    "is_list_kind": is_list_kind, "is_vector_kind": is_vector_kind, "read_vector_elem_type": read_elem_type,
    "read_elem_type": read_elem_type, "uint_byte_size": lambda t: t.byte_len, "infer_input_type": infer_input_type,
    "get_zero_value": None,   # only is_empty uses it; nothing here calls is_empty
}


def load_reference():
    """ssz_impl.py's namespace, its text executed with the two imports at its top taken out."""
    sys.path.insert(0, os.path.join(REF, "test_libs", "pyspec"))
    from eth2spec.utils import merkle_minimal
    text = open(IMPL).read()
    text, n1 = re.subn(r"^from \.\.merkle_minimal import [^\n]*\n", "", text, count=1, flags=re.M)
    text, n2 = re.subn(r"^from eth2spec\.utils\.ssz\.ssz_typing import \([^)]*\)\n", "", text, count=1, flags=re.M)
    assert n1 == 1 and n2 == 1, "ssz_impl.py's imports are not where they were"
    ns = dict(STAND_IN, merkleize_chunks=merkle_minimal.merkleize_chunks, hash=merkle_minimal.hash)
    exec(compile(text, IMPL, "exec"), ns)   # noqa: S102 -- the reference's own lines
    return ns


_types = {}


def ref_type(t):
    """The stand-in type of one of bls381_amd.ssz's type tuples."""
    key = repr(t)
    if key in _types:
        return _types[key]
    k = t[0]
    if k == "uint":
        r = _uint(t[1])
    elif k == "bool":
        r = bool
    elif k == "bytes":
        r = type("Bytes%d" % t[1], (BytesN,), {})
    elif k == "list":
        r = bytes if t[1] == S.uint(1) else SeriesType(ref_type(t[1]))
    elif k == "vector":
        r = SeriesType(ref_type(t[1]), t[2])
    else:
        r = type("C%d" % len(_types), (Container,), {"fields": tuple((name, ref_type(ft)) for name, ft in t[1])})
    _types[key] = r
    return r


def ref_value(t, v):
    k = t[0]
    if k == "uint":
        return ref_type(t)(v)
    if k == "bool":
        return bool(v)
    if k == "bytes":
        return ref_type(t)(v)
    if k in ("list", "vector"):
        return v if isinstance(v, bytes) else [ref_value(t[1], x) for x in v]
    return ref_type(t)(**{name: ref_value(ft, v[name]) for name, ft in t[1]})


BYTE_SIZES = [0, 1, 31, 32, 33, 64, 65, 512]
U64_SIZES = [0, 1, 3, 4, 5, 8, 9]
ONE = {
    "PendingAttestation": [[s] for s in BYTE_SIZES],
    "Attestation": [[0, 0], [0, 33], [33, 0], [1, 512], [31, 65], [32, 64], [64, 1], [65, 31], [512, 32]],
    "IndexedAttestation": [[0, 0], [0, 5], [5, 0], [1, 9], [3, 8], [4, 4], [8, 3], [9, 1], [4097, 3]],
    "AttesterSlashing": [[0, 0, 0, 0], [1, 3, 4, 5], [8, 9, 0, 1], [5, 0, 9, 4], [0, 8, 0, 3]],
    "BeaconBlockBody": [[0], [1, 2, 3], [2, 0, 33, 1, 65, 3], [1]],
    "BeaconBlock": [[0], [2, 1, 3, 0, 5], [1, 64, 4]],
}
LISTS = [("PendingAttestation", n, BYTE_SIZES) for n in (0, 1, 2, 3, 257, 513)] + [
    ("Attestation", 3, [33, 0, 64, 1, 512]), ("Attestation", 257, [33, 0, 64, 1, 512, 31, 65]),
    ("IndexedAttestation", 3, U64_SIZES), ("IndexedAttestation", 257, U64_SIZES),
    ("AttesterSlashing", 2, U64_SIZES), ("AttesterSlashing", 3, [5, 0, 9, 4, 1])]


def main():
    ref = load_reference()
    out = {"source": "test_libs/pyspec/eth2spec/utils/ssz/ssz_impl.py serialize / hash_tree_root / signing_root, "
                     "utils/merkle_minimal.py merkleize_chunks",
           "how": "ssz_impl.py's text executed at generation time with its two import statements replaced: "
                  "ssz_typing (which raises TypeError at import on Python 3.10) by the generator's stand-in type "
                  "layer, merkle_minimal imported as it is",
           "values": "tests/ssz_ragged_model.py Stream / value_for over bls381_amd.ssz's types: case_value(case), "
                     "list_case_values(case)",
           "items": [], "lists": []}

    def one(name, v):
        t = getattr(S, name)
        rt, rv = ref_type(t), ref_value(t, v)
        ser = ref["serialize"](rv, typ=rt)
        root = ref["hash_tree_root"](rv, typ=rt)
        assert M.serialize(t, v) == ser and M.root(t, v) == root, name
        return t, rt, rv, ser, root

    for name, size_sets in ONE.items():
        cases = [{"type": name, "seed": "%s/%d" % (name, j), "sizes": sz} for j, sz in enumerate(size_sets)]
        cases.append({"type": name, "seed": name + "/zero", "sizes": [0], "zero": True})
        for case in cases:
            t, rt, rv, ser, root = one(name, M.case_value(case))
            case.update(length=len(ser), sha256=hashlib.sha256(ser).hexdigest(), root=root.hex())
            if name == "BeaconBlock":
                case["signing_root"] = ref["signing_root"](rv, rt).hex()
                assert M.signing_root(t, M.case_value(case)).hex() == case["signing_root"]
            elif name != "BeaconBlockBody":
                assert M.root_from_bytes(t, ser) == (0, root), case
            out["items"].append(case)
            print(name, case["sizes"], len(ser), root.hex()[:16], flush=True)
    for name, n, sizes in LISTS:
        case = {"type": name, "n": n, "seed": "list/%s/%d" % (name, n), "sizes": sizes}
        t = getattr(S, name)
        values = M.list_case_values(case)
        lt = S.List(t)
        rt = ref_type(lt)
        rv = ref_value(lt, values)
        root = ref["hash_tree_root"](rv, typ=rt)
        sers = [ref["serialize"](ref_value(t, v), typ=ref_type(t)) for v in values]
        assert M.list_root(t, sers) == root
        case.update(length=sum(len(x) for x in sers), sha256=hashlib.sha256(b"".join(sers)).hexdigest(), root=root.hex())
        out["lists"].append(case)
        print("List", name, n, root.hex()[:16], flush=True)
    with open(os.path.join(HERE, "ssz_ragged.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("ssz_ragged.json:", len(out["items"]), "items,", len(out["lists"]), "lists")


if __name__ == "__main__":
    main()
