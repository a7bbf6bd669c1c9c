"""The fork choice on the GPU: bls381_fork_choice_* in both forms against fork_choice_model.py
(itself pinned to the reference's spec text by test_fork_choice_host.py) over the scripts of
fork_choice_cases.py, then the Python front and the chain committees -> attesting entries -> latest
messages -> head over a validator_registry_tree.  All results are integers or bytes and must be equal."""
import ctypes
import json
import os

import numpy as np
import pytest

import fork_choice_cases as C
import fork_choice_model as M

pytestmark = pytest.mark.gpu

GUARD = 64   # bytes of 0xEE behind every output
RECORD, OFFSETS = 121, (88, 96, 113)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fork_choice.json")


@pytest.fixture(scope="module")
def FC(native):
    from bls381_amd import fork_choice
    return fork_choice


@pytest.fixture(scope="module")
def dev(native):
    import torch

    class Dev:
        device = torch.device("cuda:0")
        L = native.lib()

        @staticmethod
        def stream():
            return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        @staticmethod
        def up(arr):
            return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).to(Dev.device)

        @staticmethod
        def out(nbytes):
            """nbytes of output with GUARD bytes behind them, all 0xEE."""
            return torch.full((int(nbytes) + GUARD,), 0xEE, dtype=torch.uint8, device=Dev.device)

        @staticmethod
        def down(t, nbytes, dtype):
            """The first nbytes as dtype; everything behind them is still 0xEE."""
            torch.cuda.synchronize()
            raw = t.cpu().numpy()
            assert np.all(raw[int(nbytes):] == 0xEE), "written past the output"
            return np.frombuffer(raw[:int(nbytes)].tobytes(), dtype=dtype)

    return Dev


def p(a, off=0):
    return ctypes.c_void_p(a.ctypes.data + off)


def arr(values, dtype):
    a = np.zeros(len(values) + 1, dtype)
    a[:len(values)] = np.asarray([int(x) for x in values], dtype=dtype) if len(values) else []
    return a


def guarded(nbytes):
    return np.full(int(nbytes) + GUARD, 0xEE, np.uint8)


def unguard(a, nbytes, dtype, rc):
    assert np.all(a[int(nbytes):] == 0xEE), "written past the output"
    if rc:
        assert np.all(a == 0xEE), "a rejected call wrote"
        return None
    return np.frombuffer(a[:int(nbytes)].tobytes(), dtype)


def records(act, ext, eff):
    n = len(eff)
    rec = np.full((max(n, 1), RECORD), 0xA5, dtype=np.uint8)
    for col, off in zip((act, ext, eff), OFFSETS):
        if n:
            rec[:n, off:off + 8] = np.asarray([int(x) for x in col], dtype="<u8").view(np.uint8).reshape(n, 8)
    return rec


class Engine:
    """The calls of a script on the engine: blocks, latest and prune through the host entry points;
    on_attestations and head through the host forms or, with `device`, the _device forms over
    tensors with guard bytes.  `use_records`: the registry as 121-byte records."""

    def __init__(self, native, dev, device, use_records):
        self.native, self.dev, self.L, self.device, self.use_records = native, dev, native.lib(), device, use_records
        self.fc = None

    def close(self):
        if self.fc:
            self.L.bls381_fork_choice_destroy(self.fc)
        self.fc = None

    def rc(self, rc):
        assert rc in (0, self.native.EARG), (rc, self.native.last_error())
        return rc

    def create(self, vcap, bcap):
        self.close()
        h = ctypes.c_void_p()
        self.native.check(self.L.bls381_fork_choice_create(vcap, bcap, ctypes.byref(h)))
        self.fc = h

    def add_blocks(self, roots, parents, slots):
        n = len(roots)
        r, pr = b"".join(bytes(x) for x in roots) + bytes(32), b"".join(bytes(x) for x in parents) + bytes(32)
        s, ids = arr(slots, np.uint64), guarded(4 * n)
        got = unguard(ids, 4 * n, np.uint32, self.rc(self.L.bls381_fork_choice_add_blocks(self.fc, n, r, pr, p(s), p(ids))))
        if got is None:
            return None
        assert [self.L.bls381_fork_choice_node(self.fc, bytes(x)) for x in roots] == got.tolist()
        return got.tolist()

    def on_attestations(self, att_off, entries, slots, targets, ok):
        n_att = len(slots)
        o, e, s, t = arr(att_off, np.uint32), arr(entries, np.uint32), arr(slots, np.uint64), arr(targets, np.uint32)
        k = arr(ok, np.uint8) if ok is not None else None
        if not self.device:
            skipped = guarded(8)
            rc = self.rc(self.L.bls381_fork_choice_on_attestations(self.fc, n_att, p(o), p(e), p(s), p(t),
                                                                   None if k is None else p(k), p(skipped)))
            got = unguard(skipped, 8, np.uint64, rc)
            return None if got is None else int(got[0])
        dev = self.dev
        d_e, d_k, d_skipped = dev.up(e), None if k is None else dev.up(k), dev.out(8)
        ws = dev.out(self.L.bls381_fork_choice_on_attestations_workspace_size(n_att))
        rc = self.rc(self.L.bls381_fork_choice_on_attestations_device(
            self.fc, n_att, p(o), d_e.data_ptr(), p(s), p(t), None if d_k is None else d_k.data_ptr(), d_skipped.data_ptr(),
            ws.data_ptr(), dev.stream()))
        if rc:
            import torch
            torch.cuda.synchronize()
            assert bool((d_skipped == 0xEE).all()), "a rejected call wrote"
            return None
        return int(dev.down(d_skipped, 8, np.uint64)[0])

    def latest(self, first, n):
        slots, targets = guarded(8 * n), guarded(4 * n)
        rc = self.rc(self.L.bls381_fork_choice_read_latest(self.fc, first, n, p(slots), p(targets)))
        a, b = unguard(slots, 8 * n, np.uint64, rc), unguard(targets, 4 * n, np.uint32, rc)
        return None if rc else (a.tolist(), b.tolist())

    def prune(self, node):
        return None if self.rc(self.L.bls381_fork_choice_prune(self.fc, node)) else True

    def head(self, start, act, ext, eff, epoch):
        n, B = len(eff), int(self.L.bls381_fork_choice_block_count(self.fc))
        if self.use_records:
            rec, stride = records(act, ext, eff), RECORD
            offs = OFFSETS
        else:
            rec, stride = np.concatenate([arr(x, np.uint64) for x in (act, ext, eff)]), 8
            offs = (0, 8 * (n + 1), 16 * (n + 1))
        if not self.device:
            head, root, weights, status = guarded(4), guarded(32), guarded(8 * B), guarded(8)
            rc = self.rc(self.L.bls381_fork_choice_head(self.fc, start, n, *[p(rec, o) for o in offs], stride, epoch, p(head),
                                                        p(root), p(weights), p(status)))
            got = [unguard(a, nb, dt, rc) for a, nb, dt in ((head, 4, np.uint32), (root, 32, np.uint8), (weights, 8 * B, np.uint64),
                                                           (status, 8, np.uint64))]
            return None if rc else (int(got[0][0]), got[1].tobytes(), got[2].tolist(), int(got[3][0]))
        dev = self.dev
        d_rec = dev.up(rec)
        d_head, d_weights, d_status = dev.out(4), dev.out(8 * B), dev.out(8)
        rc = self.rc(self.L.bls381_fork_choice_head_device(self.fc, start, n, *[d_rec.data_ptr() + o for o in offs], stride, epoch,
                                                           d_head.data_ptr(), d_weights.data_ptr(), d_status.data_ptr(),
                                                           dev.stream()))
        if rc:
            import torch
            torch.cuda.synchronize()
            assert all(bool((t == 0xEE).all()) for t in (d_head, d_weights, d_status)), "a rejected call wrote"
            return None
        head = int(dev.down(d_head, 4, np.uint32)[0])
        root = ctypes.create_string_buffer(32)
        assert self.L.bls381_fork_choice_root(self.fc, head, root) == 0
        return head, root.raw, dev.down(d_weights, 8 * B, np.uint64).tolist(), int(dev.down(d_status, 8, np.uint64)[0])


def both_forms(native, dev, scripts, want=None):
    """Every script in the device form and the host form, the registry as records in one and as
    plain arrays in the other, alternating."""
    for t, (name, script) in enumerate(scripts.items()):
        expected = want[name] if want else C.expected(script)
        for device in (True, False):
            e = Engine(native, dev, device, use_records=(t % 2 == 0) == device)
            try:
                assert C.run_script(script, e) == expected, (name, "device" if device else "host")
            finally:
                e.close()


# ------------------------------------------------------------------------------------------ the shapes
def test_validators_at_the_tile_edges(native, dev):
    """0, 1, 2047, 2048, 2049 and 4097 validators."""
    both_forms(native, dev, C.validator_size_cases())


def test_blocks_at_the_kernels_bounds(native, dev):
    """1 and 2 blocks, one below / at / one above the scan's tile and the LDS bins, the chain of
    1,025 (every round of the pointer doubling of its capacity), the comb, the star, a start node in
    the middle."""
    cases = C.block_size_cases()
    both_forms(native, dev, cases)
    assert C.expected(cases["a chain of 1025, no votes"])[-1][0] == 1024


@pytest.mark.parametrize("use_records", [False, True])
def test_a_registry_of_seventy_thousand(native, dev, use_records):
    script = C.large_registry_case()
    want = C.expected(script)
    assert sum(1 for c in want[-1][2] if c) > 20
    for device in (True, False):
        e = Engine(native, dev, device, use_records)
        try:
            assert C.run_script(script, e) == want
        finally:
            e.close()


def test_latest_messages(native, dev):
    """One validator in many attestations of a batch and across batches, a batch on one validator,
    entries out of range, verdicts with failures, the largest slot, empty attestations."""
    both_forms(native, dev, C.latest_cases())


def test_votes(native, dev):
    """All on one node, spread over every node, ties decided by one byte of the roots, sums that
    reach and pass 2^64 - 1, a start node in the middle, no validators, one block."""
    cases = C.vote_cases()
    both_forms(native, dev, cases)
    assert C.expected(cases["a sum that wraps"])[-1][3] == 3


def test_prune(native, dev):
    script, blocks, votes, reg, anchor = C.prune_cases()
    both_forms(native, dev, {"prune": script})
    # the head and counts after prune equal a fresh store fed the surviving blocks and the same log
    kept, new = C.surviving(blocks, anchor)
    tag, off, entries, slots, targets, ok = votes
    fresh = [("S", len(reg[0]), 30), C.add_call(kept),
             ("A", off, entries, slots, [new.get(t, 0) for t in targets], [t in new for t in targets]),
             ("H", 0) + reg + (C.EPOCH,)]
    for device in (True, False):
        a, b = Engine(native, dev, device, True), Engine(native, dev, device, False)
        try:
            assert C.run_script(script, a)[6] == C.run_script(fresh, b)[3]
        finally:
            a.close(), b.close()


def test_random_scripts(native, dev):
    both_forms(native, dev, {k: s for k, s in enumerate(C.random_scripts(40, seed=5))})


def test_rejected_arguments(native, dev):
    """BLS381_EARG in both forms, nothing written, and the store as it was."""
    both_forms(native, dev, C.rejected_cases())
    L, EARG = native.lib(), native.EARG
    h = ctypes.c_void_p()
    assert L.bls381_fork_choice_create(0, 8, ctypes.byref(h)) == EARG and not h
    assert L.bls381_fork_choice_create(8, 0, ctypes.byref(h)) == EARG
    assert L.bls381_fork_choice_create(1 << 32, 8, ctypes.byref(h)) == EARG
    assert L.bls381_fork_choice_create(8, (1 << 24) + 1, ctypes.byref(h)) == EARG
    assert L.bls381_fork_choice_create(8, 8, None) == EARG
    assert L.bls381_fork_choice_on_attestations_workspace_size(1 << 32) == 0
    native.check(L.bls381_fork_choice_create(8, 8, ctypes.byref(h)))
    try:
        blocks = C.chain_tree(3)
        tag, roots, parents, slots = C.add_call(blocks)
        s = arr(slots, np.uint64)
        assert L.bls381_fork_choice_add_blocks(h, 3, b"".join(roots), b"".join(parents), p(s), None) == 0
        assert L.bls381_fork_choice_add_blocks(h, 3, None, b"".join(parents), p(s), None) == EARG
        assert L.bls381_fork_choice_add_blocks(None, 3, b"".join(roots), b"".join(parents), p(s), None) == EARG
        assert L.bls381_fork_choice_node(h, bytes(32)) == M.NONE and L.bls381_fork_choice_node(None, roots[0]) == M.NONE
        assert L.bls381_fork_choice_root(h, 3, ctypes.create_string_buffer(32)) == EARG
        cols = [arr([0] * 8, np.uint64), arr([C.FAR] * 8, np.uint64), arr([C.ETH] * 8, np.uint64)]
        head, status = np.zeros(1, np.uint32), np.zeros(1, np.uint64)
        call = L.bls381_fork_choice_head
        ptrs = [p(c) for c in cols]
        assert call(h, 0, 8, *ptrs, 8, 5, p(head), None, None, p(status)) == 0 and head[0] == 2
        assert call(h, 0, 8, *ptrs, 7, 5, p(head), None, None, p(status)) == EARG
        assert call(h, 0, 8, None, *ptrs[1:], 8, 5, p(head), None, None, p(status)) == EARG
        assert call(h, 0, 8, *ptrs, 8, 5, None, None, None, p(status)) == EARG
        assert call(h, 0, 8, *ptrs, 8, 5, p(head), None, None, None) == EARG
        assert call(None, 0, 8, *ptrs, 8, 5, p(head), None, None, p(status)) == EARG
        d_cols = [dev.up(c) for c in cols]
        d_head, d_status = dev.out(8), dev.out(16)
        dcall = L.bls381_fork_choice_head_device
        dptrs = [t.data_ptr() for t in d_cols]
        assert dcall(h, 0, 8, *dptrs, 8, 5, d_head.data_ptr() + 2, None, d_status.data_ptr(), dev.stream()) == EARG
        assert dcall(h, 0, 8, *dptrs, 8, 5, d_head.data_ptr(), None, d_status.data_ptr() + 4, dev.stream()) == EARG
        assert dcall(h, 0, 8, *dptrs, 8, 5, d_head.data_ptr(), d_status.data_ptr() + 4, d_status.data_ptr(), dev.stream()) == EARG
        assert dev.down(d_head, 8, np.uint8).tolist() == [0xEE] * 8 and dev.down(d_status, 16, np.uint8).tolist() == [0xEE] * 16
        o, e, sl, t = arr([0, 2], np.uint32), dev.up(arr([1, 2], np.uint32)), arr([300], np.uint64), arr([1], np.uint32)
        acall = L.bls381_fork_choice_on_attestations_device
        ws = dev.out(L.bls381_fork_choice_on_attestations_workspace_size(1))
        d_skipped = dev.out(8)
        assert acall(h, 1, p(o), e.data_ptr(), p(sl), p(t), None, d_skipped.data_ptr() + 4, ws.data_ptr(), dev.stream()) == EARG
        assert acall(h, 1, p(o), e.data_ptr() + 2, p(sl), p(t), None, d_skipped.data_ptr(), ws.data_ptr(), dev.stream()) == EARG
        assert acall(h, 1, p(o), e.data_ptr(), p(sl), p(t), None, d_skipped.data_ptr(), None, dev.stream()) == EARG
        assert acall(h, 1, p(o), None, p(sl), p(t), None, d_skipped.data_ptr(), ws.data_ptr(), dev.stream()) == EARG
        assert acall(h, 1, None, e.data_ptr(), p(sl), p(t), None, d_skipped.data_ptr(), ws.data_ptr(), dev.stream()) == EARG
        assert dev.down(d_skipped, 8, np.uint8).tolist() == [0xEE] * 8
        slots_out, targets_out = np.zeros(8, np.uint64), np.zeros(8, np.uint32)
        assert L.bls381_fork_choice_read_latest(h, 0, 8, p(slots_out), p(targets_out)) == 0
        assert targets_out.tolist() == [M.NONE] * 8 and slots_out.tolist() == [0] * 8   # the rejected calls left no message
        assert L.bls381_fork_choice_read_latest(h, 0, 8, None, p(targets_out)) == EARG
    finally:
        L.bls381_fork_choice_destroy(h)
    L.bls381_fork_choice_destroy(None)


# ----------------------------------------------------------------------------------- the Python front
def test_golden_scenarios_through_the_python_front(FC):
    """lmd_ghost() over the scenarios of the reference's spec text: numpy in, numpy out."""
    fx = json.load(open(GOLDEN))
    maker = C.golden_maker()
    for s in fx["scenarios"]:
        sc = maker.scenario(s["seed"], s["n"], s["kind"])
        tag, off, entries, slots, targets, ok = C.batch(sc["log"])
        tag, roots, parents, block_slots = C.add_call(sc["blocks"])
        v = sc["validators"]
        head, counts = FC.lmd_ghost(roots, parents, block_slots, off, entries, slots, targets, roots[s["start"]],
                                    [x.activation_epoch for x in v], [x.exit_epoch for x in v],
                                    [x.effective_balance for x in v], fx["epoch"])
        assert head.hex() == s["head_root"] and counts.tolist() == s["vote_counts"], (s["kind"], s["n"])


def test_python_front_bounds_and_errors(FC):
    blocks = C.chain_tree(4)
    with FC.ForkChoice(16, 4) as fc:
        assert [fc.add_block(b[0], blocks[b[1]][0] if b[1] != M.NONE else bytes(32), b[2]) for b in blocks] == [0, 1, 2, 3]
        assert len(fc) == 4 and fc.node(blocks[2][0]) == 2 and fc.root(3) == blocks[3][0]
        with pytest.raises(KeyError):
            fc.node(bytes(32))
        with pytest.raises(ValueError):
            fc.add_block(C.root(1, 77), blocks[3][0], 900)               # over the capacity
        assert fc.on_attestations([0, 2], [1, 99], [2 ** 32 - 1], [blocks[1][0]]) == 1   # roots as targets; 99 skipped
        with pytest.raises(OverflowError):
            fc.on_attestations([0, 1], [2], [2 ** 32], [1])
        with pytest.raises(ValueError):
            fc.on_attestations([0, 1], [2], [5], [4])                    # an unknown target node
        slots, targets = fc.latest(0, 3)
        assert slots.tolist() == [0, 2 ** 32 - 1, 0] and targets.tolist() == [M.NONE, 1, M.NONE]
        reg = ([0] * 16, [C.FAR] * 16, [2 ** 63] * 16)
        assert fc.head(blocks[0][0], reg, 3) == blocks[3][0]
        assert fc.vote_counts().tolist() == [2 ** 63, 2 ** 63, 0, 0]
        fc.on_attestations([0, 2], [2, 3], [7], [3])
        with pytest.raises(OverflowError):
            fc.head(blocks[0][0], reg, 3)                                # 3 x 2^63 at the anchor
        assert fc.vote_counts().tolist() == [M.MAX64] * 4                # saturated, every one counted
        fc.prune(blocks[2][0])
        assert len(fc) == 2 and fc.node(blocks[3][0]) == 1
        assert fc.latest(1, 3)[1].tolist() == [M.NONE, 1, 1]


# ------------------------------------------------------------------------------------------- the chain
def test_attestations_from_committees_to_the_head(native, dev, FC):
    """Committees -> bls381_attesting_entries_device -> on_attestations_device on its d_entries (with
    its verdicts as d_ok) -> head over a validator_registry_tree's records, against the model fed the
    same attestations."""
    import torch
    from bls381_amd import committees, state_tree
    n, n_att = 600, 12
    rng = np.random.default_rng(5)
    shuffled = committees.shuffled_indices(n, bytes(range(32)), rounds=10)
    bounds = committees.committee_bounds(n, n_att)
    coff, clen = bounds[:-1].astype(np.uint32), np.diff(bounds).astype(np.uint32)
    agg, cust = [], []
    for a in range(n_att):
        bits = rng.integers(0, 2, int(clen[a])).astype(np.uint8)
        cbits = bits & rng.integers(0, 2, int(clen[a])).astype(np.uint8)
        agg.append(np.packbits(bits, bitorder="little").tobytes())
        cust.append(np.packbits(cbits, bitorder="little").tobytes())
    assert int(clen[5]) % 8
    agg[5] = agg[5][:-1] + bytes([agg[5][-1] | 0x80])   # a bit past the committee: fails verify_bitfield
    gko, ok, entries = committees.attesting_entries(shuffled, coff, clen, agg, cust)   # the host form, for the model
    assert not ok[5] and ok.sum() == n_att - 1
    blocks = C.random_tree(40, seed=91)
    slots = [300 + a % 3 for a in range(n_att)]
    targets = [int(rng.integers(20, 40)) for _ in range(n_att)]
    act, ext, eff = C.registry(n, seed=92)
    model = M.Store(n, 64)
    model.add_blocks(*C.add_call(blocks)[1:])
    att_off = [int(gko[2 * a]) for a in range(n_att)] + [int(gko[-1])]
    assert model.on_attestations(att_off, entries.tolist(), slots, targets, ok.tolist()) == 0
    want = model.head(0, act, ext, eff, C.EPOCH)
    # the device chain
    L = native.lib()
    boff = np.zeros(n_att + 1, np.uint32)
    boff[1:] = np.cumsum([len(b) for b in agg])
    d_shuffled, d_entries = dev.up(shuffled), dev.out(4 * int(clen.sum()))
    h_gko, h_ok = np.zeros(2 * n_att + 1, np.uint32), np.zeros(n_att, np.uint8)
    ws = dev.out(L.bls381_attesting_entries_workspace_size(n_att, int(boff[-1])))
    native.check(L.bls381_attesting_entries_device(n_att, p(coff), p(clen), p(boff), b"".join(agg), b"".join(cust),
                                                   d_shuffled.data_ptr(), n, p(h_gko), p(h_ok), d_entries.data_ptr(),
                                                   int(clen.sum()), ws.data_ptr(), dev.stream()))
    assert h_gko.tolist() == gko.tolist()
    d_ok = dev.up(h_ok)   # where the grouped verify's verdicts would be
    rec = records(act, ext, eff)
    rec[:, 112] = 0
    with FC.ForkChoice(n, 64) as fc, state_tree.validator_registry_tree(1024) as vt:
        vt.append([rec[i].tobytes() for i in range(n)])
        fc.add_blocks(*C.add_call(blocks)[1:])
        keep = fc.on_attestations_device(h_gko[0::2], d_entries.data_ptr(), slots, targets, d_ok.data_ptr())
        head = fc.head(blocks[0][0], vt, C.EPOCH)
        assert int(keep[0].cpu()[0]) == 0
        assert head == blocks[want[0]][0] and fc.vote_counts().tolist() == want[1]
        got_slots, got_targets = fc.latest(0, n)
        assert (got_slots.tolist(), got_targets.tolist()) == tuple(model.latest(0, n))
    torch.cuda.synchronize()
