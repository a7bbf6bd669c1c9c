"""The epoch context on the device: bls381_active_indices, bls381_active_index_root,
bls381_proposer_indices and their Python front (bls381_amd/epoch.py) against
tests/golden/epoch_context.json and the spec restated in epoch_model.py, then validator records
-> active indices -> index root -> seed -> shuffle -> proposers and attesting entries on device
buffers.  CPU half: test_epoch_host.py."""
import ctypes
import hashlib
import random

import numpy as np
import pytest

import epoch_cases as C
import epoch_model as M
import shuffle_model as SM

pytestmark = pytest.mark.gpu

GUARD = 64   # bytes of 0xEE behind every device output


def cvp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def epoch(native):
    from bls381_amd import epoch
    return epoch


@pytest.fixture(scope="module")
def fx():
    return M.fixture()


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
        def ws(nbytes):
            return torch.full((max(int(nbytes), 1),), 0xEE, dtype=torch.uint8, device=Dev.device)

        @staticmethod
        def down(t, nbytes, dtype):
            """The first nbytes as dtype; everything behind them is still 0xEE."""
            raw = t.cpu().numpy()
            assert np.all(raw[int(nbytes):] == 0xEE), "written past the output"
            return np.frombuffer(raw[:int(nbytes)].tobytes(), dtype=dtype)

    return Dev


def dev_active(dev, n, d_act, d_ext, stride, ep, d_bal=None, bal_stride=8):
    """The _device form on torch buffers (pointers as ints): (indices, total)."""
    import torch
    L = dev.L
    d_idx, d_ct = dev.out(4 * n), dev.out(16)
    ws = dev.ws(L.bls381_active_indices_workspace_size(n))
    rc = L.bls381_active_indices_device(n, d_act, d_ext, stride, ep, d_bal, bal_stride, d_idx.data_ptr(), d_ct.data_ptr(),
                                        ws.data_ptr(), dev.stream())
    assert rc == 0
    torch.cuda.synchronize()
    count, total = (int(v) for v in dev.down(d_ct, 16, np.uint64))
    return dev.down(d_idx, 4 * count, np.uint32), total


def host_active(native, n, act, ext, ep, bal=None):
    """The host-pointer form: (indices, total); nothing is written past the count."""
    out = np.full(n + 1, 0xEEEEEEEE, dtype=np.uint32)
    count, total = ctypes.c_uint64(99), ctypes.c_uint64(99)
    native.check(native.lib().bls381_active_indices(n, cvp(act), cvp(ext), 8, ep, None if bal is None else cvp(bal), 8,
                                                    cvp(out), ctypes.byref(count), ctypes.byref(total)))
    assert np.all(out[count.value:] == 0xEEEEEEEE)
    return out[:count.value], total.value


# ------------------------------------------------------------------------- active indices
@pytest.mark.parametrize("n", C.ACTIVE_SIZES)
def test_active_indices_patterns(native, dev, n):
    bal = C.balances(n)
    d_bal = dev.up(bal)
    for name, (act, ext, ep) in C.active_patterns(n).items():
        want = C.expected_active(act, ext, ep)
        total = C.expected_total(bal, want)
        got, t = host_active(native, n, act, ext, ep, bal)
        assert np.array_equal(got, want) and t == total, name
        d_act, d_ext = dev.up(act), dev.up(ext)
        got, t = dev_active(dev, n, d_act.data_ptr(), d_ext.data_ptr(), 8, ep, d_bal.data_ptr())
        assert np.array_equal(got, want) and t == total, name
    act, ext, ep = C.active_patterns(n)["mixed"]
    got, t = host_active(native, n, act, ext, ep)                 # no balances: no sum
    assert np.array_equal(got, C.expected_active(act, ext, ep)) and t == 0


def test_active_indices_fixture_and_front(epoch, fx):
    for case in fx["cases"]:
        for e in case["epochs"]:
            got, total = epoch.active_validator_indices(case["activation_epochs"], case["exit_epochs"], e["epoch"],
                                                        case["effective_balances"])
            assert got.dtype == np.uint32 and got.tolist() == e["active"]
            assert max(total, 1) == e["total_balance"]


def test_active_indices_513_tiles(native, dev):
    """2^20 + 3 validators: the scan's workgroup loops three times over the tile counts."""
    n = C.ACTIVE_LARGE
    rng = np.random.default_rng(5)
    act = rng.choice(np.array([0, 5, 6, C.FAR], dtype=np.uint64), n)
    ext = rng.choice(np.array([C.FAR, 5, 6, 2 ** 63], dtype=np.uint64), n)
    bal = rng.integers(0, 33, n).astype(np.uint64) * np.uint64(C.ETH)
    want = np.flatnonzero((act <= np.uint64(5)) & (np.uint64(5) < ext)).astype(np.uint32)
    total = int(bal[want].sum(dtype=np.uint64))
    got, t = host_active(native, n, act, ext, 5, bal)
    assert np.array_equal(got, want) and t == total
    d_act, d_ext, d_bal = dev.up(act), dev.up(ext), dev.up(bal)
    got, t = dev_active(dev, n, d_act.data_ptr(), d_ext.data_ptr(), 8, 5, d_bal.data_ptr())
    assert np.array_equal(got, want) and t == total


@pytest.mark.parametrize("n", [1, 65, 257, 2049])
def test_active_indices_over_validator_records(native, dev, n):
    """Stride 121 at an odd base, host and device forms; the buffers end with the last field."""
    act, ext, ep = C.active_patterns(n)["mixed"]
    bal = C.balances(n)
    buf, base = C.records_at_odd_base(act, ext, bal)
    tight = buf[:base + (n - 1) * M.VALIDATOR_BYTES + M.OFF_BALANCE + 8].copy()
    want = C.expected_active(act, ext, ep)
    total = C.expected_total(bal, want)
    out = np.full(n + 1, 0xEEEEEEEE, dtype=np.uint32)
    count, tot = ctypes.c_uint64(0), ctypes.c_uint64(0)
    at = lambda off: ctypes.c_void_p(tight.ctypes.data + base + off)  # noqa: E731
    native.check(dev.L.bls381_active_indices(n, at(M.OFF_ACTIVATION), at(M.OFF_EXIT), M.VALIDATOR_BYTES, ep,
                                             at(M.OFF_BALANCE), M.VALIDATOR_BYTES, cvp(out), ctypes.byref(count),
                                             ctypes.byref(tot)))
    assert np.array_equal(out[:count.value], want) and out[count.value] == 0xEEEEEEEE and tot.value == total
    d = dev.up(tight)
    p0 = d.data_ptr() + base
    got, t = dev_active(dev, n, p0 + M.OFF_ACTIVATION, p0 + M.OFF_EXIT, M.VALIDATOR_BYTES, ep, p0 + M.OFF_BALANCE,
                        M.VALIDATOR_BYTES)
    assert np.array_equal(got, want) and t == total


def test_active_indices_arguments(native, dev):
    import torch
    L, E = dev.L, native.EARG
    a = C.u64([0, 0])
    d = dev.up(a)
    d_idx, d_ct, ws = dev.out(64), dev.out(16), dev.ws(L.bls381_active_indices_workspace_size(2))
    sp = dev.stream()

    def call(n=2, act=d.data_ptr(), ext=d.data_ptr(), stride=8, bal=None, bstride=8, idx=d_idx.data_ptr(),
             ct=d_ct.data_ptr(), w=ws.data_ptr()):
        return L.bls381_active_indices_device(n, act, ext, stride, 0, bal, bstride, idx, ct, w, sp)

    assert call() == 0
    assert call(n=1 << 32) == E and L.bls381_active_indices_workspace_size(1 << 32) == 0
    assert call(stride=7) == E and call(bal=d.data_ptr(), bstride=7) == E
    assert call(act=None) == E and call(ext=None) == E and call(idx=None) == E and call(ct=None) == E and call(w=None) == E
    assert call(idx=d_idx.data_ptr() + 2) == E and call(ct=d_ct.data_ptr() + 4) == E
    # n == 0: the count is written as 0, nothing else is needed
    d_ct0 = dev.out(16)
    assert call(n=0, act=None, ext=None, idx=None, w=None, ct=d_ct0.data_ptr()) == 0
    torch.cuda.synchronize()
    assert dev.down(d_ct0, 16, np.uint64).tolist() == [0, 0]
    out = np.zeros(2, dtype=np.uint32)
    cnt = ctypes.c_uint64(7)
    assert L.bls381_active_indices(0, None, None, 8, 0, None, 8, None, ctypes.byref(cnt), None) == 0 and cnt.value == 0
    assert L.bls381_active_indices(2, cvp(a), cvp(a), 8, 0, None, 8, cvp(out), None, None) == E
    assert L.bls381_active_indices(2, None, cvp(a), 8, 0, None, 8, cvp(out), ctypes.byref(cnt), None) == E
    assert L.bls381_active_indices(2, cvp(a), cvp(a), 4, 0, None, 8, cvp(out), ctypes.byref(cnt), None) == E
    assert L.bls381_active_indices(1 << 32, cvp(a), cvp(a), 8, 0, None, 8, cvp(out), ctypes.byref(cnt), None) == E


# ---------------------------------------------------------------------------- index root
def dev_root(dev, idx):
    import torch
    L = dev.L
    n = len(idx)
    d_idx, d_root = dev.up(idx) if n else None, dev.out(32)
    ws = dev.ws(L.bls381_active_index_root_workspace_size(n))
    assert L.bls381_active_index_root_device(n, d_idx.data_ptr() if n else None, d_root.data_ptr(), ws.data_ptr(),
                                             dev.stream()) == 0
    torch.cuda.synchronize()
    return dev.down(d_root, 32, np.uint8).tobytes()


@pytest.mark.parametrize("n", C.ROOT_SIZES)
def test_index_root(native, dev, epoch, n):
    from bls381_amd import ssz
    rng = random.Random(n)
    idx = np.array(sorted(rng.sample(range(1 << 32), n)), dtype=np.uint32)
    want = M.active_index_root(idx.tolist())
    assert epoch.active_index_root(idx) == want
    assert dev_root(dev, idx) == want
    assert ssz.hash_tree_root(ssz.List(ssz.uint(8)), idx.tolist()) == want


def test_index_root_large(dev, epoch):
    n = C.ACTIVE_LARGE
    idx = (np.arange(n, dtype=np.uint64) * np.uint64(4093) % np.uint64(1 << 32)).astype(np.uint32)
    # the model's tree, level by level in numpy-sized steps
    data = idx.astype("<u8").tobytes()
    data += bytes(-len(data) % 32)
    layer = [data[k:k + 32] for k in range(0, len(data), 32)]
    want = hashlib.sha256(M.merkleize(layer) + n.to_bytes(32, "little")).digest()
    assert epoch.active_index_root(idx) == want
    assert dev_root(dev, idx) == want


def test_index_roots_of_the_fixture(epoch, fx):
    for case in fx["cases"]:
        for e in case["epochs"]:
            assert epoch.active_index_root(e["active"]).hex() == e["index_root"]


def test_index_root_arguments(native, dev):
    L, E = dev.L, native.EARG
    idx = np.arange(5, dtype=np.uint32)
    d_idx, d_root, ws = dev.up(idx), dev.out(32), dev.ws(L.bls381_active_index_root_workspace_size(5))
    sp = dev.stream()
    assert L.bls381_active_index_root_device(1 << 32, d_idx.data_ptr(), d_root.data_ptr(), ws.data_ptr(), sp) == E
    assert L.bls381_active_index_root_workspace_size(1 << 32) == 0
    assert L.bls381_active_index_root_device(5, None, d_root.data_ptr(), ws.data_ptr(), sp) == E
    assert L.bls381_active_index_root_device(5, d_idx.data_ptr(), None, ws.data_ptr(), sp) == E
    assert L.bls381_active_index_root_device(5, d_idx.data_ptr(), d_root.data_ptr(), None, sp) == E
    assert L.bls381_active_index_root_device(5, d_idx.data_ptr() + 1, d_root.data_ptr(), ws.data_ptr(), sp) == E
    root = np.zeros(32, dtype=np.uint8)
    assert L.bls381_active_index_root(5, None, cvp(root)) == E and L.bls381_active_index_root(5, cvp(idx), None) == E
    assert L.bls381_active_index_root(0, None, cvp(root)) == 0
    assert root.tobytes() == hashlib.sha256(bytes(64)).digest()      # mix_in_length(zero chunk, 0)


# ----------------------------------------------------------------------------- proposers
def dev_proposers(dev, shuffled, coff, clen, bal, seed, ep, max_eb=C.MAX_EB, n_validators=None):
    import torch
    L = dev.L
    coff, clen = np.asarray(coff, dtype=np.uint32), np.asarray(clen, dtype=np.uint32)
    d_sh, d_bal, d_out = dev.up(shuffled), dev.up(bal), dev.out(4 * len(coff))
    ws = dev.ws(L.bls381_proposer_indices_workspace_size(len(coff)))
    assert L.bls381_proposer_indices_device(len(coff), cvp(coff), cvp(clen), d_sh.data_ptr(), len(shuffled),
                                            d_bal.data_ptr(), 8, len(bal) if n_validators is None else n_validators, seed,
                                            ep, max_eb, d_out.data_ptr(), ws.data_ptr(), dev.stream()) == 0
    torch.cuda.synchronize()
    return dev.down(d_out, 4 * len(coff), np.uint32).tolist()


def both_proposers(dev, epoch, shuffled, coff, clen, bal, seed, ep, max_eb=C.MAX_EB):
    got = epoch.beacon_proposer_indices(shuffled, coff, clen, bal, seed, ep, max_eb).tolist()
    assert dev_proposers(dev, shuffled, coff, clen, bal, seed, ep, max_eb) == got
    return got


def test_proposers_of_the_fixture(dev, epoch, fx):
    for case in fx["cases"]:
        consts = fx["supplied"]["constants"][case["preset"]]
        st = M.fixture_state(case, consts)
        committees = case.get("committees") or [M.get_crosslink_committee(st, 5, s) for s in case["shards"]]
        per_slot = len(committees) // consts["SLOTS_PER_EPOCH"]
        shuffled = np.array([v for m in committees for v in m], dtype=np.uint32)
        bounds = np.concatenate([[0], np.cumsum([len(m) for m in committees])])
        slots = [s for s, want in enumerate(case["proposers"]) if want is not None]
        if not slots:
            continue
        coff = [bounds[per_slot * s] for s in slots]
        clen = [len(committees[per_slot * s]) for s in slots]
        got = both_proposers(dev, epoch, shuffled, coff, clen, C.u64(case["effective_balances"]),
                             bytes.fromhex(case["seed"]), 5, consts["MAX_EFFECTIVE_BALANCE"])
        assert got == [case["proposers"][s] for s in slots], (case["preset"], case["n"])


def test_proposer_full_balances_win_at_try_zero(dev, epoch):
    bal = C.u64([C.MAX_EB] * 50)
    shuffled = C.committee_of(60, 50)
    for ep in (0, 7, 2 ** 40 + 3):
        got = both_proposers(dev, epoch, shuffled, [0, 3, 10], [1, 3, 50], bal, hashlib.sha256(b"full").digest(), ep)
        assert got == [int(shuffled[0]), int(shuffled[3 + ep % 3]), int(shuffled[10 + ep % 50])]


@pytest.mark.parametrize("want", C.WINNING_TRIES + ["late"])
def test_proposer_winning_try_at_digest_and_window_edges(dev, epoch, want):
    """Balances all 0: the winning try is the seed's first zero random byte, found on the CPU;
    committees of 1, 3 and 4,096 with epoch % len != 0 in one call."""
    seed, t = C.seed_with_winning_try(want)
    bal = C.u64([0] * 100)
    shuffled = C.committee_of(1 + 3 + 4096, 100)
    coff, clen, ep = [0, 1, 4], [1, 3, 4096], 4099
    assert ep % 3 and ep % 4096
    expect = [M.proposer_search(shuffled[o:o + l].tolist(), ep, bal.tolist(), seed, C.MAX_EB) for o, l in zip(coff, clen)]
    assert all(e[1] == t for e in expect)
    assert both_proposers(dev, epoch, shuffled, coff, clen, bal, seed, ep) == [e[0] for e in expect]


def test_64_slots_in_one_call(dev, epoch):
    rng = random.Random(0x64)
    nv = 5000
    bal = C.u64([rng.choice([0, 1, 8, 16, 31, 32, 40]) * C.ETH + rng.randrange(3) for _ in range(nv)])
    shuffled = C.committee_of(64 * 128 + 5, nv)
    coff = [128 * s + (s % 5) for s in range(64)]
    clen = [128 - (s % 7) for s in range(64)]
    seed, ep = hashlib.sha256(b"64 slots").digest(), 2 ** 33 + 11
    want = [M.proposer_search(shuffled[o:o + l].tolist(), ep, bal.tolist(), seed, C.MAX_EB)[0] for o, l in zip(coff, clen)]
    assert both_proposers(dev, epoch, shuffled, coff, clen, bal, seed, ep) == want


def test_proposer_out_of_range_entry(dev, epoch):
    """An entry >= n_validators met before the winning try gives 0xFFFFFFFF for its slot only; the
    balances end with the last validator (the buffer's guard is intact, and nothing beyond is read)."""
    seed, t = C.seed_with_winning_try(31)
    bal = C.u64([0] * 4)
    shuffled = np.array([0, 1, 4, 3, 0, 1, 0xFFFFFFFF, 3, 0, 1, 2, 3] + [0] * 40 + [99], dtype=np.uint32)
    got = both_proposers(dev, epoch, shuffled, [0, 4, 8, 12], [4, 4, 4, 41], bal, seed, 0)
    assert got == [0xFFFFFFFF, 0xFFFFFFFF, 3, 0]    # slot 2: try 31 -> member 31 % 4; slot 3: member 99 never reached


def test_proposer_arguments(native, dev):
    L, E = dev.L, native.EARG
    sh, bal = np.arange(8, dtype=np.uint32), C.u64([C.MAX_EB] * 8)
    d_sh, d_bal, d_out = dev.up(sh), dev.up(bal), dev.out(8)
    ws = dev.ws(L.bls381_proposer_indices_workspace_size(2))
    seed = bytes(32)

    def call(n=2, off=(0, 4), ln=(4, 4), shp=d_sh.data_ptr(), nsh=8, balp=d_bal.data_ptr(), bstride=8, nv=8, sd=seed,
             max_eb=C.MAX_EB, outp=d_out.data_ptr(), w=ws.data_ptr()):
        o, l = np.array(off, dtype=np.uint32), np.array(ln, dtype=np.uint32)
        return L.bls381_proposer_indices_device(n, cvp(o), cvp(l), shp, nsh, balp, bstride, nv, sd, 3, max_eb, outp, w,
                                                dev.stream())

    assert call() == 0
    assert call(ln=(4, 0)) == E and call(off=(0, 5)) == E and call(nsh=7) == E          # empty / outside n_shuffled
    assert call(max_eb=0) == E and call(max_eb=2 ** 56) == E and call(max_eb=2 ** 56 - 1) == 0
    assert call(bstride=7) == E and call(nv=1 << 32) == E
    assert call(shp=None) == E and call(balp=None) == E and call(sd=None) == E and call(outp=None) == E and call(w=None) == E
    assert call(shp=d_sh.data_ptr() + 2) == E and call(outp=d_out.data_ptr() + 1) == E
    assert L.bls381_proposer_indices_workspace_size(1 << 31) == 0
    assert L.bls381_proposer_indices_device(0, None, None, None, 0, None, 8, 0, None, 0, C.MAX_EB, None, None, dev.stream()) == 0
    assert L.bls381_proposer_indices(0, None, None, None, 0, None, 8, 0, None, 0, C.MAX_EB, None) == 0
    out = np.zeros(2, dtype=np.uint32)
    o, l = np.array([0, 4], dtype=np.uint32), np.array([4, 0], dtype=np.uint32)
    assert L.bls381_proposer_indices(2, cvp(o), cvp(l), cvp(sh), 8, cvp(bal), 8, 8, seed, 3, C.MAX_EB, cvp(out)) == E
    l[1] = 4
    assert L.bls381_proposer_indices(2, cvp(o), cvp(l), cvp(sh), 8, cvp(bal), 8, 8, seed, 3, 0, cvp(out)) == E
    assert L.bls381_proposer_indices(2, cvp(o), cvp(l), cvp(sh), 8, cvp(bal), 8, 8, seed, 3, C.MAX_EB, cvp(out)) == 0
    assert out.tolist() == [3, 7]       # full balances: try 0, member epoch % 4
    import torch
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ the chain
def test_epoch_committees_front(epoch, fx):
    for case in fx["cases"]:
        k = fx["supplied"]["constants"][case["preset"]]
        ec = epoch.EpochCommittees(case["activation_epochs"], case["exit_epochs"], case["effective_balances"], 5,
                                   bytes.fromhex(case["randao_mix"]), case["epochs"][1]["start_shard"],
                                   shard_count=k["SHARD_COUNT"], slots_per_epoch=k["SLOTS_PER_EPOCH"],
                                   target_committee_size=k["TARGET_COMMITTEE_SIZE"],
                                   shuffle_round_count=k["SHUFFLE_ROUND_COUNT"],
                                   max_effective_balance=k["MAX_EFFECTIVE_BALANCE"])
        assert ec.seed.hex() == case["seed"] and ec.committee_count == case["epochs"][1]["committee_count"]
        got = [ec.crosslink_committee(s).tolist() for s in case["shards"]]
        assert [len(m) for m in got] == case["committee_lengths"]
        assert SM.list_digest([v for m in got for v in m]) == case["committees_sha256"]
        assert [None if v == epoch.PROPOSER_NONE else int(v) for v in ec.proposers()] == case["proposers"]
        st = M.fixture_state(case, k)
        count_at = lambda e: M.active_count(st, e)  # noqa: E731
        for e in case["epochs"]:
            assert epoch.epoch_start_shard(case["latest_start_shard"], 5, e["epoch"], count_at, k["SHARD_COUNT"],
                                           k["SLOTS_PER_EPOCH"], k["TARGET_COMMITTEE_SIZE"]) == e["start_shard"]
            assert epoch.shard_delta(len(e["active"]), k["SHARD_COUNT"], k["SLOTS_PER_EPOCH"],
                                     k["TARGET_COMMITTEE_SIZE"]) == e["shard_delta"]


def test_records_to_committees_and_proposers_on_device_buffers(native, dev, fx):
    """A minimal-preset epoch with the validator records in device memory: active indices -> index
    root -> seed (96 bytes on the host) -> shuffle with the gather -> proposers and attesting
    entries, one host read of the count; every shard's committee and every slot's proposer equal
    the model's."""
    import torch
    L = dev.L
    k = fx["supplied"]["constants"]["minimal"]
    rng = random.Random(0xC4A1)
    n, ep = 200, 5
    act = [rng.choice([0, 0, 0, 5, 6, C.FAR]) for _ in range(n)]
    ext = [rng.choice([C.FAR, C.FAR, C.FAR, 5, 6, 2 ** 63]) for _ in range(n)]
    bal = [rng.choice([0, 8, 16, 31, 32, 32]) * C.ETH for _ in range(n)]
    mix = hashlib.sha256(b"chain mix").digest()
    st = M.State(act, ext, bal, ep * k["SLOTS_PER_EPOCH"], 3, mix, k)
    shards = [(M.epoch_start_shard(st, ep) + j) % k["SHARD_COUNT"] for j in range(M.epoch_committee_count(M.active_count(st, ep), k))]
    model_committees = [M.get_crosslink_committee(st, ep, s) for s in shards]
    model_proposers = []
    for s in range(k["SLOTS_PER_EPOCH"]):
        st.slot = ep * k["SLOTS_PER_EPOCH"] + s
        model_proposers.append(M.get_beacon_proposer_index(st))

    sp = dev.stream()
    buf, base = C.records_at_odd_base(C.u64(act), C.u64(ext), C.u64(bal))
    d_rec = dev.up(buf)
    p0 = d_rec.data_ptr() + base
    d_idx, d_ct, d_root = dev.out(4 * n), dev.out(16), dev.out(32)
    aws = dev.ws(L.bls381_active_indices_workspace_size(n))
    native.check(L.bls381_active_indices_device(n, p0 + M.OFF_ACTIVATION, p0 + M.OFF_EXIT, M.VALIDATOR_BYTES, ep,
                                                p0 + M.OFF_BALANCE, M.VALIDATOR_BYTES, d_idx.data_ptr(), d_ct.data_ptr(),
                                                aws.data_ptr(), sp))
    count = int(dev.down(d_ct, 16, np.uint64)[0])                 # the chain's one host read
    assert count == M.active_count(st, ep)
    rws = dev.ws(L.bls381_active_index_root_workspace_size(count))
    native.check(L.bls381_active_index_root_device(count, d_idx.data_ptr(), d_root.data_ptr(), rws.data_ptr(), sp))
    torch.cuda.synchronize()
    from bls381_amd import epoch as E
    seed = E.generate_seed(mix, dev.down(d_root, 32, np.uint8).tobytes(), ep)
    assert seed == M.state_seed(st, ep)
    rounds = k["SHUFFLE_ROUND_COUNT"]
    d_sh = dev.out(4 * count)
    sws = dev.ws(L.bls381_shuffle_workspace_size(count, count, rounds))
    native.check(L.bls381_shuffle_device(count, seed, rounds, 0, count, d_idx.data_ptr(), d_sh.data_ptr(), sws.data_ptr(), sp))
    ncom = len(shards)
    bounds = [(count * j) // ncom for j in range(ncom + 1)]
    per_slot = ncom // k["SLOTS_PER_EPOCH"]
    coff = np.array([bounds[per_slot * s] for s in range(k["SLOTS_PER_EPOCH"])], dtype=np.uint32)
    clen = np.array([bounds[per_slot * s + 1] - bounds[per_slot * s] for s in range(k["SLOTS_PER_EPOCH"])], dtype=np.uint32)
    d_prop = dev.out(4 * len(coff))
    pws = dev.ws(L.bls381_proposer_indices_workspace_size(len(coff)))
    native.check(L.bls381_proposer_indices_device(len(coff), cvp(coff), cvp(clen), d_sh.data_ptr(), count,
                                                  p0 + M.OFF_BALANCE, M.VALIDATOR_BYTES, n, seed, ep,
                                                  k["MAX_EFFECTIVE_BALANCE"], d_prop.data_ptr(), pws.data_ptr(), sp))
    # one attestation per committee, every member attesting, no custody bits
    aoff = np.array(bounds[:-1], dtype=np.uint32)
    alen = np.array([bounds[j + 1] - bounds[j] for j in range(ncom)], dtype=np.uint32)
    bits = [bytes([0xFF] * (l // 8) + ([(1 << (l % 8)) - 1] if l % 8 else [])) for l in alen.tolist()]
    boff = np.concatenate([[0], np.cumsum([len(b) for b in bits])]).astype(np.uint32)
    gko, ok = np.zeros(2 * ncom + 1, dtype=np.uint32), np.zeros(ncom, dtype=np.uint8)
    d_ent = dev.out(4 * count)
    ews = dev.ws(L.bls381_attesting_entries_workspace_size(ncom, int(boff[-1])))
    native.check(L.bls381_attesting_entries_device(ncom, cvp(aoff), cvp(alen), cvp(boff), b"".join(bits), bytes(int(boff[-1])),
                                                   d_sh.data_ptr(), count, cvp(gko), cvp(ok), d_ent.data_ptr(), count,
                                                   ews.data_ptr(), sp))
    torch.cuda.synchronize()
    shuffled = dev.down(d_sh, 4 * count, np.uint32).tolist()
    assert [shuffled[bounds[j]:bounds[j + 1]] for j in range(ncom)] == model_committees
    assert dev.down(d_prop, 4 * len(coff), np.uint32).tolist() == model_proposers
    entries = dev.down(d_ent, 4 * count, np.uint32).tolist()
    assert ok.tolist() == [1] * ncom
    assert [entries[gko[2 * j]:gko[2 * j + 1]] for j in range(ncom)] == [sorted(m) for m in model_committees]
