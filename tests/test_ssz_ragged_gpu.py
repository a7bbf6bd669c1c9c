"""Roots of variable-size SSZ containers on the device: k_ssz_ragged_root through
both forms of the C ABI against ssz_ragged_model.py and tests/golden/ssz_ragged.json, malformed
items, rejected arguments, the list root, RaggedListTree, and the paths of bls381_amd.ssz that now
take one call.  CPU half (the model against the fixture, the host build): test_ssz_ragged_host.py."""
import ctypes
import json
import os

import numpy as np
import pytest

import ssz_ragged_model as M
from bls381_amd import ssz as S

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssz_ragged.json")
RAGGED = ("PendingAttestation", "Attestation", "IndexedAttestation", "AttesterSlashing")
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def fx():
    return json.load(open(GOLDEN))


@pytest.fixture(scope="module")
def items(fx):
    """{type name: [(serialized item, root)]}: the fixture's single items, the model's bytes."""
    out = {}
    for case in fx["items"]:
        if case["type"] in RAGGED:
            t = getattr(S, case["type"])
            out.setdefault(case["type"], []).append((M.serialize(t, M.case_value(case)), bytes.fromhex(case["root"])))
    return out


@pytest.fixture(scope="module")
def lists(fx):
    """[(case, type, serialized elements)] of the fixture's lists, built once."""
    return [(c, getattr(S, c["type"]), [M.serialize(getattr(S, c["type"]), v) for v in M.list_case_values(c)])
            for c in fx["lists"]]


def p(a):
    return a.ctypes.data_as(vp)


def starts_of(sers):
    starts = np.zeros(len(sers) + 1, dtype=np.uint64)
    np.cumsum([len(x) for x in sers], out=starts[1:])
    return starts


def device_roots(native, typ, sers, starts=None, items_bytes=None):
    """(rc, roots, status, n_bad) of bls381_ssz_ragged_roots_device over torch buffers."""
    import torch
    L = native.lib()
    n = len(sers)
    blob = b"".join(sers)
    starts = starts_of(sers) if starts is None else starts
    prog = S.compile_root(typ)
    d_items = torch.frombuffer(bytearray(blob or b"\x00"), dtype=torch.uint8).cuda()
    d_starts = torch.from_numpy(starts.astype(np.int64)).cuda()
    d_roots = torch.full((32 * max(n, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    d_status = torch.full((max(n, 1),), 0xEE, dtype=torch.uint8, device="cuda")
    d_bad = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    ws = torch.empty(max(1, L.bls381_ssz_ragged_roots_workspace_size(n)), dtype=torch.uint8, device="cuda")
    rc = L.bls381_ssz_ragged_roots_device(n, d_items.data_ptr(), len(blob) if items_bytes is None else items_bytes,
                                          d_starts.data_ptr(), p(prog), len(prog), d_roots.data_ptr(),
                                          d_status.data_ptr(), d_bad.data_ptr(), ws.data_ptr(),
                                          vp(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    raw = bytes(d_roots.cpu().numpy())
    return rc, [raw[32 * i:32 * i + 32] for i in range(n)], d_status.cpu().numpy()[:n], int(d_bad.item())


def device_list_root(native, typ, sers):
    import torch
    L = native.lib()
    n = len(sers)
    blob = b"".join(sers)
    prog = S.compile_root(typ)
    d_items = torch.frombuffer(bytearray(blob or b"\x00"), dtype=torch.uint8).cuda()
    d_starts = torch.from_numpy(starts_of(sers).astype(np.int64)).cuda()
    d_root = torch.zeros(32, dtype=torch.uint8, device="cuda")
    d_bad = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    ws = torch.empty(max(1, L.bls381_ssz_ragged_list_root_workspace_size(n)), dtype=torch.uint8, device="cuda")
    rc = L.bls381_ssz_ragged_list_root_device(n, d_items.data_ptr(), len(blob), d_starts.data_ptr(), p(prog), len(prog),
                                              1, d_root.data_ptr(), d_bad.data_ptr(), ws.data_ptr(),
                                              vp(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, bytes(d_root.cpu().numpy()), int(d_bad.item())


def test_both_forms_match_the_model(native, items):
    """Every fixture item of every ragged type, the 1,025-chunk index list among them, in one batch
    per type: neighbouring lanes run different field lengths."""
    for name in RAGGED:
        t = getattr(S, name)
        sers = [s for s, _ in items[name]]
        want = [r for _, r in items[name]]
        assert [M.root_from_bytes(t, s) for s in sers] == [(0, r) for r in want]
        roots, status = S.hash_tree_root_ragged_batch(t, sers)
        assert roots == want and not status.any(), name
        rc, roots, status, bad = device_roots(native, t, sers)
        assert (rc, roots, bad) == (0, want, 0) and not status.any(), name


def test_malformed_items_are_isolated(native, items):
    """Each rule broken in turn among good items: status 1 and a zero root for it, the neighbours'
    roots unchanged, the bad count right -- the host form and the device form."""
    for name in RAGGED:
        t = getattr(S, name)
        good = [s for s, _ in items[name]][1:4]
        bad = [item for _, item in M.malformed(t, good[0])]
        batch = []
        for k, item in enumerate(bad):          # good, bad, good, bad, ...
            batch += [good[k % 3], item]
        batch.append(good[1])
        want = [M.root_from_bytes(t, x) for x in batch]
        assert sum(st for st, _ in want) == len(bad)
        roots, status = S.hash_tree_root_ragged_batch(t, batch)
        assert list(zip(status.tolist(), roots)) == want, name
        rc, roots, status, n_bad = device_roots(native, t, batch)
        assert rc == 0 and list(zip(status.tolist(), roots)) == want and n_bad == len(bad), name
        with pytest.raises(ValueError):
            S.list_root_ragged(t, batch)
        rc, _, n_bad = device_list_root(native, t, batch)
        assert (rc, n_bad) == (0, len(bad))
        bad_count = ctypes.c_uint32(77)
        out = ctypes.create_string_buffer(b"\x55" * 32, 32)
        prog = S.compile_root(t)
        rc = native.lib().bls381_ssz_ragged_list_root(len(batch), b"".join(batch), p(starts_of(batch)), p(prog), len(prog), 1,
                                                      out, ctypes.byref(bad_count))
        assert (rc, bad_count.value, out.raw) == (native.EARG, len(bad), b"\x55" * 32)


def test_device_ranges_that_are_no_items(native, items):
    """Device-side offsets cannot be checked on the host: a decreasing range and one past the buffer
    are malformed items, and nothing is read for them."""
    t = S.Attestation
    sers = [s for s, _ in items["Attestation"]][:4]
    want = [r for _, r in items["Attestation"]][:4]
    starts = starts_of(sers)
    broken = starts.copy()
    broken[2] = starts[1] - 1                 # item 1 decreases; item 2 then starts inside item 1: malformed or not, by the model
    rc, roots, status, n_bad = device_roots(native, t, sers, broken)
    blob = b"".join(sers)
    model = [M.root_from_bytes(t, blob[int(broken[i]):int(broken[i + 1])]) if broken[i] <= broken[i + 1] else (1, bytes(32))
             for i in range(4)]
    assert rc == 0 and list(zip(status.tolist(), roots)) == model and n_bad == sum(st for st, _ in model)
    assert model[0] == (0, want[0]) and model[3] == (0, want[3]) and model[1][0] == 1
    # the buffer ends inside the last item
    rc, roots, status, n_bad = device_roots(native, t, sers, items_bytes=len(blob) - 1)
    assert rc == 0 and roots[:3] == want[:3] and status.tolist() == [0, 0, 0, 1] and roots[3] == bytes(32) and n_bad == 1


def test_no_items(native):
    t = S.PendingAttestation
    roots, status = S.hash_tree_root_ragged_batch(t, [])
    assert roots == [] and len(status) == 0
    empty = M.mix_in_length(M.ZERO[0], 0)
    assert S.list_root_ragged(t, []) == empty
    assert S.list_root_ragged(t, [], mix_length=False) == M.ZERO[0]
    assert device_list_root(native, t, []) == (0, empty, 0)
    prog = S.compile_root(t)
    out = ctypes.create_string_buffer(32)
    assert native.lib().bls381_ssz_ragged_list_root(0, None, None, p(prog), len(prog), 1, out, None) == 0
    assert out.raw == empty
    assert native.lib().bls381_ssz_ragged_roots(0, None, None, p(prog), len(prog), None, None) == 0


def test_rejected_arguments(native, items):
    L = native.lib()
    t = S.Attestation
    sers = [s for s, _ in items["Attestation"]][:3]
    blob, starts, prog = b"".join(sers), starts_of(sers), S.compile_root(t)
    out, status, root = ctypes.create_string_buffer(96), np.zeros(3, dtype=np.uint8), ctypes.create_string_buffer(32)

    def roots(n=3, blob=blob, starts=starts, prog=prog, plen=None, out=out, status=status):
        return L.bls381_ssz_ragged_roots(n, blob, None if starts is None else p(starts), p(prog),
                                         len(prog) if plen is None else plen, out, None if status is None else p(status))

    def list_root(n=3, blob=blob, starts=starts, prog=prog, root=root):
        return L.bls381_ssz_ragged_list_root(n, blob, None if starts is None else p(starts), p(prog), len(prog), 1, root, None)

    assert roots() == 0 and list_root() == 0
    fixed_prog = S.compile_root(S.Fork)                                   # not a ragged program
    bad_word = prog.copy()
    bad_word[3] = S.fixed_part_size(t) - 3                                # an offset word outside the fixed part
    down = starts.copy()
    down[1], down[2] = starts[2], starts[1]                               # non-monotone
    huge = starts.copy()
    huge[3] = starts[2] + (1 << 32)                                       # an item of 2^32 bytes
    for kw in (dict(prog=fixed_prog), dict(prog=bad_word), dict(plen=len(prog) - 1), dict(starts=down), dict(starts=huge),
               dict(blob=None), dict(starts=None), dict(out=None), dict(status=None)):
        assert roots(**kw) == native.EARG, kw
    for kw in (dict(prog=fixed_prog), dict(prog=bad_word), dict(starts=down), dict(starts=huge), dict(blob=None),
               dict(starts=None), dict(root=None)):
        assert list_root(**kw) == native.EARG, kw
    # the device forms: the same program checks, null and misaligned pointers; nothing is queued
    import torch
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    a = buf.data_ptr()
    s = vp(torch.cuda.current_stream().cuda_stream)
    assert L.bls381_ssz_ragged_roots_device(3, a, 64, a + 512, p(fixed_prog), len(fixed_prog), a + 1024, a + 2048, a + 3072,
                                            a + 3584, s) == native.EARG
    for args in ((3, a, 64, None, p(prog), len(prog), a + 1024, a + 2048, a + 3072, a + 3584, s),
                 (3, a, 64, a + 516, p(prog), len(prog), a + 1024, a + 2048, a + 3072, a + 3584, s),
                 (3, a, 64, a + 512, p(prog), len(prog), a + 1025, a + 2048, a + 3072, a + 3584, s),
                 (3, a, 64, a + 512, p(prog), len(prog), a + 1024, a + 2048, None, a + 3584, s),
                 (3, a, 64, a + 512, p(prog), len(prog), a + 1024, a + 2048, a + 3072, None, s)):
        assert L.bls381_ssz_ragged_roots_device(*args) == native.EARG, args
    assert L.bls381_ssz_ragged_list_root_device(3, a, 64, a + 512, p(prog), len(prog), 1, None, a + 3072, a + 3584,
                                                s) == native.EARG
    assert L.bls381_ssz_ragged_list_root_workspace_size(1 << 31) == 0 and L.bls381_ssz_ragged_roots_workspace_size(1 << 31) == 0


def test_list_root_matches_the_fixture(native, lists):
    """Lists of 0, 1, 2, 3, 257 and 513 elements (the tile edges of the reduction), mixed field lengths."""
    for case, t, sers in lists:
        want = bytes.fromhex(case["root"])
        assert S.list_root_ragged(t, sers) == want, case
        assert device_list_root(native, t, sers) == (0, want, 0), case


def test_ragged_list_tree(native, lists):
    """Appended in three uneven batches it equals the one-call list root and the fixture; a
    malformed batch leaves it unchanged; clear() restores the empty root; replace() the whole list."""
    from bls381_amd.state_tree import RaggedListTree
    case, t, sers = next(x for x in lists if x[0]["type"] == "PendingAttestation" and x[0]["n"] == 257)
    empty = M.mix_in_length(M.ZERO[0], 0)
    with RaggedListTree(300, t) as tree:
        assert tree.root() == empty and len(tree) == 0
        tree.append(sers[:5])
        assert tree.root() == M.list_root(t, sers[:5])
        tree.append(sers[5:200])
        before = tree.root()
        bad = M.malformed(t, sers[0])[2][1]
        with pytest.raises(ValueError):
            tree.append(sers[200:210] + [bad] + sers[211:220])
        assert tree.root() == before and len(tree) == 200
        with pytest.raises(ValueError):
            tree.append(sers[:101])              # does not fit
        assert tree.root() == before and len(tree) == 200
        tree.append(sers[200:])
        assert tree.root() == bytes.fromhex(case["root"]) == S.list_root_ragged(t, sers) and len(tree) == 257
        with pytest.raises(ValueError):
            tree.replace([bad])
        assert tree.root() == bytes.fromhex(case["root"])
        tree.replace(sers[:3])
        assert tree.root() == M.list_root(t, sers[:3]) and len(tree) == 3
        tree.clear()
        assert tree.root() == empty and len(tree) == 0
        tree.append(sers[:2])
        assert tree.root() == M.list_root(t, sers[:2])
    with pytest.raises(ValueError):
        RaggedListTree(8, S.Fork)


def test_series_root_takes_one_call_with_the_same_bytes(native, fx):
    """List(PendingAttestation) of 5 elements: hash_tree_root through the new path equals the
    per-element path -- the element roots field by field and merkle_root over them -- and the model."""
    t = S.PendingAttestation
    case = {"type": "PendingAttestation", "n": 5, "seed": "series", "sizes": [33, 0, 512, 1, 64]}
    values = M.list_case_values(case)
    new = S.hash_tree_root(S.List(t), values)

    def element_root(v):        # the path of the parent commit: a call per field, one to combine them
        roots = [S.hash_tree_root(ft, v[name]) for name, ft in t[1]]
        return S.merkle_root(roots, S.chunk_depth(len(roots)))

    old = S.merkle_root([element_root(v) for v in values], S.chunk_depth(5), 0, 5)
    assert new == old == M.root(S.List(t), values)
    assert S.hash_tree_root(t, values[0]) == element_root(values[0])


def test_block_body_and_block_roots(native, fx):
    """hash_tree_root(BeaconBlockBody) and signing_root(BeaconBlock) equal the fixture."""
    for case in fx["items"]:
        if case["type"] == "BeaconBlockBody":
            assert S.hash_tree_root(S.BeaconBlockBody, M.case_value(case)).hex() == case["root"], case
        if case["type"] == "BeaconBlock":
            v = M.case_value(case)
            assert S.signing_root(S.BeaconBlock, v).hex() == case["signing_root"], case
            assert S.hash_tree_root(S.BeaconBlock, v).hex() == case["root"], case
