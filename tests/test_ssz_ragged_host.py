"""Roots of variable-size SSZ containers on the CPU: ssz_ragged_model.py against
tests/golden/ssz_ragged.json (the reference's own ssz_impl lines, make_ssz_ragged_vectors.py), then
the code one lane of k_ssz_ragged_root runs (csrc/bls381_ssz.hpp ssz_run_ragged, host build) against
the model, the host check of a program, the Python side (serialize, compile_root), and the same
header in a stand-alone ASan/UBSan program.  GPU half: test_ssz_ragged_gpu.py, which also holds
hash_tree_root(BeaconBlockBody) and signing_root(BeaconBlock): the engine has no CPU fallback."""
import ctypes
import hashlib
import itertools
import json
import os
import random
import subprocess

import numpy as np
import pytest

import ssz_ragged_model as M
from bls381_amd import ssz as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssz_ragged.json")
RAGGED = ("PendingAttestation", "Attestation", "IndexedAttestation", "AttesterSlashing")
vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64


@pytest.fixture(scope="module")
def fx():
    return json.load(open(GOLDEN))


@pytest.fixture(scope="module")
def L():
    import build_native
    lib = ctypes.CDLL(os.environ.get("BLS381_HOSTCHECK_LIB") or build_native.build_hostcheck())
    lib.hc_ssz_ragged_root.argtypes = [vp, u32, vp, u32, vp]
    lib.hc_ssz_ragged_root.restype = ctypes.c_int
    lib.hc_ssz_ragged_prog_ok.argtypes = [vp, u32, u64]
    lib.hc_ssz_ragged_prog_ok.restype = ctypes.c_int
    return lib


def host_root(L, prog, item: bytes):
    """(rc, root) of the host build for one item, held in a buffer of exactly its bytes."""
    prog = np.ascontiguousarray(prog, dtype=np.uint32)
    buf = (ctypes.c_uint8 * len(item)).from_buffer_copy(item) if item else None
    out = ctypes.create_string_buffer(32)
    rc = L.hc_ssz_ragged_root(buf, len(item), prog.ctypes.data_as(vp), len(prog), out)
    return rc, out.raw


def prog_ok(L, prog, max_field_bytes=0):
    prog = np.ascontiguousarray(prog, dtype=np.uint32)
    return bool(L.hc_ssz_ragged_prog_ok(prog.ctypes.data_as(vp), len(prog), max_field_bytes))


def fixture_items(fx, names=RAGGED):
    """[(type name, type, serialized item, root)] of the fixture's single items."""
    out = []
    for case in fx["items"]:
        if case["type"] in names:
            t = getattr(S, case["type"])
            out.append((case["type"], t, M.serialize(t, M.case_value(case)), bytes.fromhex(case["root"])))
    return out


def random_items(count=320, seed=0x55A):
    """Seeded random items of the four ragged types, most fields short, some past a chunk boundary."""
    rng = random.Random(seed)
    out = []
    for i in range(count):
        name = RAGGED[i % 4]
        t = getattr(S, name)
        sizes = [rng.choice([0, 1, 2, 7, 31, 32, 33, 63, 64, 65, 100, rng.randrange(300)]) for _ in range(4)]
        out.append((name, t, M.serialize(t, M.value_for(t, M.Stream("rnd/%d" % i), itertools.cycle(sizes)))))
    return out


def test_model_matches_the_fixture(fx):
    """The model's serialization and roots are the reference's, from values and from bytes."""
    assert "ssz_impl.py" in fx["source"] and "stand-in" in fx["how"]
    assert {c["type"] for c in fx["items"]} == set(RAGGED) | {"BeaconBlockBody", "BeaconBlock"}
    for case in fx["items"]:
        t, v = getattr(S, case["type"]), M.case_value(case)
        ser = M.serialize(t, v)
        assert (len(ser), hashlib.sha256(ser).hexdigest()) == (case["length"], case["sha256"]), case
        assert M.root(t, v).hex() == case["root"], case
        if case["type"] in RAGGED:
            assert M.root_from_bytes(t, ser) == (0, bytes.fromhex(case["root"])), case
        if "signing_root" in case:
            assert M.signing_root(t, v).hex() == case["signing_root"], case
    assert sorted(c["n"] for c in fx["lists"] if c["type"] == "PendingAttestation") == [0, 1, 2, 3, 257, 513]
    for case in fx["lists"]:
        t = getattr(S, case["type"])
        sers = [M.serialize(t, v) for v in M.list_case_values(case)]
        assert hashlib.sha256(b"".join(sers)).hexdigest() == case["sha256"], case
        assert M.list_root(t, sers).hex() == case["root"], case


def test_fixture_covers_the_edges(fx):
    """The field lengths the code can go wrong at are in the fixture: chunk edges of a bytes field,
    chunk edges of a uint64 list, 1,025 chunks once, both fields empty, one of two empty."""
    sizes = {name: [tuple(c["sizes"]) for c in fx["items"] if c["type"] == name and not c.get("zero")] for name in RAGGED}
    assert {s[0] for s in sizes["PendingAttestation"]} == {0, 1, 31, 32, 33, 64, 65, 512}
    for name, want in (("Attestation", {0, 1, 31, 32, 33, 64, 65, 512}), ("IndexedAttestation", {0, 1, 3, 4, 5, 8, 9, 4097})):
        assert {x for s in sizes[name] for x in s} == want
        assert (0, 0) in sizes[name] and any(a == 0 < b for a, b in sizes[name]) and any(b == 0 < a for a, b in sizes[name])
    assert sum(4097 in s for s in sizes["IndexedAttestation"]) == 1
    assert any(len(set(s)) == 4 for s in sizes["AttesterSlashing"])
    assert all(any(c.get("zero") for c in fx["items"] if c["type"] == name) for name in RAGGED)


def test_host_build_matches_the_model(L, fx):
    for name, t, ser, root in fixture_items(fx):
        assert host_root(L, S.compile_root(t), ser) == (0, root), name
    for name, t, ser in random_items():
        assert host_root(L, S.compile_root(t), ser) == M.root_from_bytes(t, ser), name


def test_host_build_on_corrupted_fixed_parts(L):
    """Random bytes written over the fixed part -- the offsets among them -- and random truncations:
    status and root as the model's, whatever the offsets then say."""
    rng = random.Random(0xC0FFEE)
    bad = 0
    for name, t, ser in random_items(240, seed=7):
        b = bytearray(ser)
        for pos in M.offset_positions(t):
            if rng.random() < 0.6:
                b[pos:pos + 4] = rng.choice([rng.randrange(len(ser) + 40), rng.randrange(1 << 32)]).to_bytes(4, "little")
        if rng.random() < 0.3:
            b = b[:rng.randrange(len(b) + 1)]
        want = M.root_from_bytes(t, bytes(b))
        bad += want[0]
        assert host_root(L, S.compile_root(t), bytes(b)) == want, name
    assert 40 < bad < 240


def test_each_rule_broken_in_turn(L, fx):
    """Status 1 and a zero root for each rule, and the items before and after keep their roots."""
    for name in RAGGED:
        t = getattr(S, name)
        prog = S.compile_root(t)
        good = [ser for n, _, ser, _ in fixture_items(fx, (name,))][1:3]
        want = [M.root_from_bytes(t, g) for g in good]
        for label, item in M.malformed(t, good[0]):
            got = [host_root(L, prog, x) for x in (good[0], item, good[1])]
            assert got == [want[0], (1, b"\x00" * 32), want[1]], (name, label)


def test_prog_ok_accepts_and_rejects(L):
    for name in RAGGED:
        prog = list(S.compile_root(getattr(S, name)))
        assert prog_ok(L, prog) and S.ragged_prog_ok(prog), name
    R, C, Mk, F, E, Lv, NO = S.SSZ_RAGGED, S.SSZ_CHUNK, S.SSZ_MERKLE, S.SSZ_FIELD, S.SSZ_ENTER, S.SSZ_LEAVE, S.SSZ_NO_NEXT
    ok = [R, 12, F, 0, NO, 1, C, 4, 8, Mk, 2]
    cases = [
        (ok, 0, True),
        ([C, 0, 8], 0, False),                                         # not a ragged program
        ([R, 12, F, 0, NO, 1, C, 5, 8, Mk, 2], 0, False),              # chunk read past the fixed part
        ([R, 12, F, 9, NO, 1, C, 4, 8, Mk, 2], 0, False),              # offset word outside the fixed part
        ([R, 12, F, 0, 10, 1, C, 4, 8, Mk, 2], 0, False),              # the next offset word outside it
        ([R, 12, F, 0, NO, 3, C, 4, 8, Mk, 2], 0, False),              # element size no power of two
        ([R, 12, F, 0, NO, 64, C, 4, 8, Mk, 2], 0, False),             # element size above a chunk
        ([R, 12, F, 0, NO, 1, C, 4, 8], 0, False),                     # two chunks left
        ([R, (1 << 16) + 1, F, 0, NO, 1], 0, False),                   # fixed part too large
        ([R, 4, F, 0, NO, 1, Lv], 0, False),                           # leave without enter
        ([R, 4, E, 0, NO, 4, F, 0, NO, 1], 0, False),                  # enter without leave
        ([R, 4, E, 0, NO, 4, F, 0, NO, 1, Lv], 0, True),
        ([R, 4] + [E, 0, NO, 4] * 3 + [F, 0, NO, 1] + [Lv] * 3, 0, True),    # scopes 4 deep
        ([R, 4] + [E, 0, NO, 4] * 4 + [F, 0, NO, 1] + [Lv] * 4, 0, False),   # 5 deep
        # the stack peak: 36 chunks below a field leave 28 entries, what the longest field needs ...
        ([R, 8] + [C, 4, 4] * 36 + [F, 0, NO, 1, Mk, 37], 0, True),
        ([R, 8] + [C, 4, 4] * 37 + [F, 0, NO, 1, Mk, 38], 0, False),         # ... 37 do not
        ([R, 8] + [C, 4, 4] * 37 + [F, 0, NO, 1, Mk, 38], 1 << 30, True),    # 2^25 chunks: 26 entries
        ([R, 8] + [C, 4, 4] * 53 + [F, 0, NO, 1, Mk, 54], 32768, True),      # 1,024 chunks: 11 entries
        ([R, 8] + [C, 4, 4] * 54 + [F, 0, NO, 1, Mk, 55], 32768, False),
        ([R, 8] + [C, 4, 4] * 63 + [F, 0, NO, 1, Mk, 64], 32, True),         # one chunk: one entry, the 64th
    ]
    for prog, max_field, want in cases:
        assert prog_ok(L, prog, max_field) == want, (prog[:12], max_field)
        assert S.ragged_prog_ok(prog, max_field) == want, (prog[:12], max_field)
    # the host build refuses to run what the check rejects
    assert host_root(L, [R, 12, F, 9, NO, 1, C, 4, 8, Mk, 2], bytes(12))[0] == 2


def test_long_field_streams_in_few_stack_entries(L):
    """A 1,025-chunk field under 36 chunks of stack: the stream keeps one node per level."""
    R, C, Mk, F, NO = S.SSZ_RAGGED, S.SSZ_CHUNK, S.SSZ_MERKLE, S.SSZ_FIELD, S.SSZ_NO_NEXT
    data = M.Stream("long").bytes(32 * 1024 + 5)
    item = (8).to_bytes(4, "little") + b"\x07\x00\x00\x00" + data
    prog = [R, 8] + [C, 4, 4] * 36 + [F, 0, NO, 1, Mk, 37]
    leaves = [b"\x07" + bytes(31)] * 36 + [M.mix_in_length(M.merkleize(M.chunkify(data)), len(data))]
    assert host_root(L, prog, item) == (0, M.merkleize(leaves))


def test_serialize_and_compile_root(L, fx):
    """ssz.serialize gives the reference's bytes for every new type; compile_root gives programs
    the engine's check accepts for the ragged ones and refuses the block body (lists of containers)."""
    for case in fx["items"]:
        t = getattr(S, case["type"])
        ser = S.serialize(t, M.case_value(case))
        assert (len(ser), hashlib.sha256(ser).hexdigest()) == (case["length"], case["sha256"]), case
    for case in fx["lists"][:4]:
        t = getattr(S, case["type"])
        values = M.list_case_values(case)
        blob = b"".join(S.serialize(t, v) for v in values)
        assert hashlib.sha256(blob).hexdigest() == case["sha256"], case
        # the list's own serialization: an offset per element, then the elements
        assert S.serialize(S.List(t), values) == M.serialize(S.List(t), values)
    assert [int(x) for x in S.compile_root(S.PendingAttestation)[:6]] == [S.SSZ_RAGGED, 220, S.SSZ_FIELD, 0, S.SSZ_NO_NEXT, 1]
    assert [int(x) for x in S.compile_root(S.AttesterSlashing)[:10]] == [
        S.SSZ_RAGGED, 8, S.SSZ_ENTER, 0, 4, 304, S.SSZ_FIELD, 0, 4, 8]
    for name in RAGGED:
        assert S._ragged_fits(getattr(S, name)) and not S._program_fits(getattr(S, name))
    for t in (S.BeaconBlockBody, S.BeaconBlock):
        assert not S._ragged_fits(t)
        with pytest.raises(ValueError):
            S.compile_root(t)
    # fixed-size types compile as before
    assert list(S.compile_root(S.Fork)) == [1, 0, 4, 1, 4, 4, 1, 8, 8, 2, 3]


def test_sanitizer_program(L, fx, tmp_path):
    """The stand-alone ASan/UBSan build of the same header over the fixture items, every malformed
    case and the program checks, each item in a heap block of exactly its bytes."""
    import build_native
    exe = build_native.build_ssz_ragged_check()
    lines = []
    for name in RAGGED:
        t = getattr(S, name)
        prog = [int(x) for x in S.compile_root(t)]
        lines.append("P %d %s" % (len(prog), " ".join(map(str, prog))))
        sers = [ser for n, _, ser, _ in fixture_items(fx, (name,))]
        items = sers + [item for _, item in M.malformed(t, sers[1])] + [item for _, item in M.malformed(t, sers[-1])]
        for item in items:
            st, root = M.root_from_bytes(t, item)
            lines.append("I %d %s %d %s" % (len(item), item.hex() or "-", st, root.hex()))
        lines.append("K 0 1 %d %s" % (len(prog), " ".join(map(str, prog))))
        lines.append("K 0 0 %d %s" % (len(prog) - 1, " ".join(map(str, prog[:-1]))))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    run = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.split()[:4] == [str(len(lines)), "cases,", "0", "mismatches"], run.stdout
