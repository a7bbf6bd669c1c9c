"""The registry updates on the GPU: bls381_registry_updates / bls381_exit_queue in both forms
against registry_updates_model.py (itself pinned to the reference's spec text by
test_registry_updates_host.py) over the crafted registries of registry_updates_cases.py, then the
Python front over a validator_registry_tree.  All results are integers and must be equal."""
import ctypes
import json
import os

import numpy as np
import pytest

import registry_updates_cases as C
import registry_updates_model as M

pytestmark = pytest.mark.gpu

GUARD = 64   # bytes of 0xEE behind every device output
OFFSETS = (80, 88, 96, 104, 113)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "registry_updates.json")


@pytest.fixture(scope="module")
def RU(native):
    from bls381_amd import registry_updates
    return registry_updates


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


def constants(RU, case):
    return RU.RegistryConstants(*M.constants6(case["c"]))


def records(case):
    n = case["n"]
    rec = np.full((max(n, 1), 121), 0xA5, dtype=np.uint8)
    for f, off in zip(C.FIELDS, OFFSETS):
        if n:
            rec[:n, off:off + 8] = np.ascontiguousarray(case[f], dtype="<u8").view(np.uint8).reshape(n, 8)
    return rec


def device_fields(dev, case, use_records):
    """The five field pointers, the stride and the tensors to keep."""
    if use_records:
        rec = dev.up(records(case))
        return [rec.data_ptr() + off for off in OFFSETS], 121, [rec]
    keep = [dev.up(np.append(case[f], np.uint64(0))) for f in C.FIELDS]
    return [t.data_ptr() for t in keep], 8, keep


def device_call(dev, RU, case, use_records):
    """bls381_registry_updates_device: (rc, indices, values, summary)."""
    n = case["n"]
    ptrs, stride, keep = device_fields(dev, case, use_records)
    d_idx, d_val, d_sum = dev.out(4 * n), dev.out(32 * n), dev.out(64)
    ws = dev.out(dev.L.bls381_registry_updates_workspace_size(n))
    k = constants(RU, case)
    rc = dev.L.bls381_registry_updates_device(n, *ptrs, stride, case["cur"], case["fin"], ctypes.byref(k), d_idx.data_ptr(),
                                              d_val.data_ptr(), d_sum.data_ptr(), ws.data_ptr(), dev.stream())
    if rc:
        return rc, None, None, None
    return (0, dev.down(d_idx, 4 * n, np.uint32), dev.down(d_val, 32 * n, np.uint64).reshape(n, 4),
            [int(x) for x in dev.down(d_sum, 64, np.uint64)])


def host_call(native, RU, case, use_records):
    """bls381_registry_updates on host pointers with guard bytes of its own: (rc, indices, values, summary)."""
    n = case["n"]
    if use_records:
        rec = records(case)
        ptrs, stride = [ctypes.c_void_p(rec.ctypes.data + off) for off in OFFSETS], 121
    else:
        cols = [np.append(case[f], np.uint64(0)) for f in C.FIELDS]
        ptrs, stride = [ctypes.c_void_p(a.ctypes.data) for a in cols], 8
    idx, val, summary = (np.full(nbytes + GUARD, 0xEE, np.uint8) for nbytes in (4 * n, 32 * n, 64))
    k = constants(RU, case)
    rc = native.lib().bls381_registry_updates(n, *ptrs, stride, case["cur"], case["fin"], ctypes.byref(k),
                                              ctypes.c_void_p(idx.ctypes.data), ctypes.c_void_p(val.ctypes.data),
                                              ctypes.c_void_p(summary.ctypes.data))
    for a, nbytes in ((idx, 4 * n), (val, 32 * n), (summary, 64)):
        assert np.all(a[nbytes:] == 0xEE), "written past the output"
    if rc:
        assert np.all(idx == 0xEE) and np.all(val == 0xEE) and np.all(summary == 0xEE), "a rejected call wrote"
        return rc, None, None, None
    return (0, np.frombuffer(idx[:4 * n].tobytes(), np.uint32), np.frombuffer(val[:32 * n].tobytes(), np.uint64).reshape(n, 4),
            [int(x) for x in np.frombuffer(summary[:64].tobytes(), np.uint64)])


def same(case, got, want):
    rc, idx, values, summary = got
    assert rc == 0, case["name"]
    assert summary == want[2], case["name"]
    assert np.array_equal(idx, np.array(want[0], dtype=np.uint32)), case["name"]
    assert np.array_equal(values, np.array(want[1], dtype=np.uint64).reshape(case["n"], 4)), case["name"]


def both_forms(native, dev, RU, cases):
    for t, case in enumerate(cases):
        want = case.expected()
        assert want is not None, case["name"]
        same(case, device_call(dev, RU, case, use_records=t % 2 == 0), want)
        same(case, host_call(native, RU, case, use_records=t % 2 == 1), want)


# ------------------------------------------------------------------------------------ the cases
def test_sizes_at_the_tile_edges(native, dev, RU):
    """n = 0, 1, 2047, 2048, 2049, 4097 over records and plain arrays; n = 0 writes the summary alone."""
    cases = C.size_cases()
    both_forms(native, dev, RU, cases)
    both_forms(native, dev, RU, cases[1:] + cases[:1])   # the other layout for each form
    assert cases[0].expected()[2] == [0, 0, 0, 0, 0, 4, C.DELAYED_CUR, 0]


def test_second_round_of_the_tile_scan(native, dev, RU):
    """257 tiles over plain arrays, ejections and candidates on both sides of tile 256."""
    case = C.second_scan_round_case()
    n = case["n"]
    want = case.expected()
    # validator n - 1 is tile 256: the fourth ejection and the seventh, last dequeued candidate
    assert want[2][1] == 4 and want[2][5] == 7 and want[0][n - 1] == n - 1 and want[0][100] == M.NONE
    same(case, device_call(dev, RU, case, use_records=False), case.expected())
    same(case, host_call(native, RU, case, use_records=False), case.expected())


def test_exit_queue_before_the_call(native, dev, RU):
    both_forms(native, dev, RU, C.exit_queue_cases() + C.ejection_edge_cases())


def test_activation_queue(native, dev, RU):
    both_forms(native, dev, RU, C.activation_queue_cases())


def test_churn_limits(native, dev, RU):
    """L = 4 is every other test; here L = 12, L = 341 (more than one digit's bins) and L >= K."""
    both_forms(native, dev, RU, C.churn_limit_cases())


def test_wrapping_epochs(native, dev, RU):
    cases = C.overflow_cases()
    both_forms(native, dev, RU, cases)
    rc, idx, values, summary = device_call(dev, RU, cases[0], use_records=True)
    assert summary[7] == 1 and int(values[3][2]) == int(values[3][3]) == M.FAR


def test_random_registries(native, dev, RU):
    both_forms(native, dev, RU, C.random_cases(60, seed=3))


def test_golden_states_through_the_python_front(RU):
    """registry_updates() over the states of the reference's spec text: numpy in, numpy out."""
    fx = json.load(open(GOLDEN))
    for s in fx["states"]:
        if s["n"] >= fx["digest_from"]:
            continue
        ins = s["inputs"]
        k = RU.RegistryConstants.from_preset(s["constants"])
        idx, values, summary = RU.registry_updates(ins["activation_eligibility_epoch"], ins["activation_epoch"], ins["exit_epoch"],
                                                   ins["withdrawable_epoch"], ins["effective_balance"], fx["epoch"],
                                                   fx["finalized_epoch"], k)
        for x, f in enumerate(("activation_eligibility_epoch", "activation_epoch", "exit_epoch", "withdrawable_epoch")):
            assert values[:, x].tolist() == s["outputs"][f], (s["preset"], s["overrides"], s["n"], f)
        assert summary.churn_limit == s["churn_limit"] and summary.status == 0


def test_rejected_arguments(native, dev, RU):
    """BLS381_EARG in both forms; the host form also for a churn limit of 0 that only the data shows,
    which the device form reports in the status word with no change written."""
    cases = C.rejected_cases()
    for case in cases:
        assert case.expected() is None
        assert host_call(native, RU, case, use_records=False)[0] == native.EARG, case["name"]
        if case["name"] != "no churn limit that the data shows":
            assert device_call(dev, RU, case, use_records=False)[0] == native.EARG, case["name"]
    case = cases[-1]
    rc, idx, values, summary = device_call(dev, RU, case, use_records=True)
    assert rc == 0 and summary == [0, 0, 0, 0, 10, 0, C.DELAYED_CUR, RU.STATUS_NO_CHURN]
    assert np.all(idx == M.NONE)
    assert values.tolist() == [list(row) for row in zip(*case.lists()[:4])]
    # pointers and sizes
    ok = C.Case("plain", 8)
    k = constants(RU, ok)
    cols = [np.append(ok[f], np.uint64(0)) for f in C.FIELDS]
    ptrs = [ctypes.c_void_p(a.ctypes.data) for a in cols]
    idx, val, summary = np.zeros(8, np.uint32), np.zeros(32, np.uint64), np.zeros(8, np.uint64)
    outs = [ctypes.c_void_p(a.ctypes.data) for a in (idx, val, summary)]
    call = native.lib().bls381_registry_updates
    assert call(8, *ptrs, 8, 100, 90, ctypes.byref(k), *outs) == 0
    assert call(8, *ptrs, 7, 100, 90, ctypes.byref(k), *outs) == native.EARG
    assert call(8, *ptrs, 8, 100, 90, None, *outs) == native.EARG
    assert call(8, *ptrs, 8, 100, 90, ctypes.byref(k), outs[0], outs[1], None) == native.EARG
    assert call(8, *ptrs, 8, 100, 90, ctypes.byref(k), None, outs[1], outs[2]) == native.EARG
    assert call(8, None, *ptrs[1:], 8, 100, 90, ctypes.byref(k), *outs) == native.EARG
    assert call(1 << 32, *ptrs, 8, 100, 90, ctypes.byref(k), *outs) == native.EARG
    assert native.lib().bls381_registry_updates_workspace_size(1 << 32) == 0
    d_sum, ws = dev.out(64), dev.out(native.lib().bls381_registry_updates_workspace_size(8))
    dcall = native.lib().bls381_registry_updates_device
    assert dcall(0, *[None] * 5, 8, 100, 90, ctypes.byref(k), None, None, d_sum.data_ptr() + 4, ws.data_ptr(),
                 dev.stream()) == native.EARG
    assert dcall(0, *[None] * 5, 8, 100, 90, ctypes.byref(k), None, None, d_sum.data_ptr(), None, dev.stream()) == native.EARG
    assert dcall(0, *[None] * 5, 8, 100, 90, ctypes.byref(k), None, None, d_sum.data_ptr(), ws.data_ptr(), dev.stream()) == 0
    assert [int(x) for x in dev.down(d_sum, 64, np.uint64)] == [0, 0, 0, 0, 0, 4, 105, 0]


# -------------------------------------------------------------------------------- the exit queue
def test_exit_queue_both_forms(native, dev, RU):
    cases = C.exit_queue_cases() + C.size_cases() + [C.churn_limit_cases()[0]] + C.random_cases(20, seed=8)
    for t, case in enumerate(cases):
        act, ext = case.lists()[1:3]
        want = list(M.exit_queue(act, ext, case["cur"], case["c"]))
        k = constants(RU, case)
        ptrs, stride, keep = device_fields(dev, case, use_records=t % 2 == 0)
        d_q, ws = dev.out(32), dev.out(dev.L.bls381_registry_updates_workspace_size(case["n"]))
        assert dev.L.bls381_exit_queue_device(case["n"], ptrs[1], ptrs[2], stride, case["cur"], ctypes.byref(k), d_q.data_ptr(),
                                              ws.data_ptr(), dev.stream()) == 0
        assert [int(x) for x in dev.down(d_q, 32, np.uint64)] == want, case["name"]
        q = RU.exit_queue(case["act"], case["ext"], case["cur"], k)
        assert [q.epoch, q.churn, q.churn_limit, q.active_count] == want, case["name"]
    rejected = C.rejected_cases()
    for case in (rejected[0], rejected[3], rejected[5]):
        with pytest.raises(ValueError):
            RU.exit_queue(case["act"], case["ext"], case["cur"], constants(RU, case))


def test_exit_queue_initiate_gives_the_spec_texts_sequence(RU):
    """exit_queue() and ExitQueue.initiate() against repeated initiate_validator_exit of the spec text."""
    fx = json.load(open(GOLDEN))
    seen = 0
    for s in fx["states"]:
        if s["n"] >= fx["digest_from"]:
            continue
        k = RU.RegistryConstants.from_preset(s["constants"])
        q = RU.exit_queue(s["inputs"]["activation_epoch"], s["inputs"]["exit_epoch"], fx["epoch"], k)
        assert q.churn_limit == s["churn_limit"]
        for _, ex, wd in s["exits"]:
            assert q.initiate() == (ex, wd)
            seen += 1
    assert seen > 30


# ------------------------------------------------------------------------------------- the tree
def test_process_registry_updates_over_the_tree(native, dev, RU):
    """Records in a validator_registry_tree -> process_registry_updates: the tree's root equals the
    root of the model's records, and bls381_active_indices_device at delayed(cur) sees the new
    activations."""
    import list_tree_cases as LT
    from bls381_amd import state_tree
    case = C.churn_limit_cases()[0]          # L = 12, 30 ejections, a queue of 22
    n, cur, fin = case["n"], case["cur"], case["fin"]
    k = constants(RU, case)
    rec = records(case)
    rec[:, 112] = np.arange(len(rec)) % 5 == 0    # `slashed` is a bool to the tree's model
    items = [rec[i].tobytes() for i in range(n)]
    idx, values, summary = case.expected()
    with state_tree.validator_registry_tree(512) as vt:
        vt.append(items)
        q = RU.ExitQueue.of_tree(vt, cur, k)
        assert [q.epoch, q.churn, q.churn_limit, q.active_count] == list(M.exit_queue(*case.lists()[1:3], cur, case["c"]))
        got = RU.process_registry_updates(vt, cur, fin, k)
        assert list(got) == summary and got.activated == 12 and got.ejected == 30
        LT.apply_update(items, range(n), 80, 32, [b"".join(int(x).to_bytes(8, "little") for x in row) for row in values])
        assert vt.root() == LT.Model(LT.VALIDATOR, items).root(True)
        assert vt.read(0, n) == items
        at = C.DELAYED_CUR
        p = vt.items_ptr
        d_idx, d_ct = dev.out(4 * n), dev.out(16)
        aws = dev.out(dev.L.bls381_active_indices_workspace_size(n))
        native.check(dev.L.bls381_active_indices_device(n, p + 88, p + 96, 121, at, None, 0, d_idx.data_ptr(), d_ct.data_ptr(),
                                                        aws.data_ptr(), dev.stream()))
        count = int(dev.down(d_ct, 16, np.uint64)[0])
        active = dev.down(d_idx, 4 * n, np.uint32)[:count].tolist()
        assert active == [i for i, row in enumerate(values) if row[1] <= at < row[2]]
        activated = [i for i, row in enumerate(values) if row[1] != int(case["act"][i])]
        assert len(activated) == 12 and set(activated) <= set(active)
        # six epochs on, finality has passed the first batch: the rest of the queue follows
        cur2, fin2 = cur + 6, cur + 1
        lists2 = [[row[x] for row in values] for x in range(4)] + [case.lists()[4]]
        idx2, values2, summary2 = M.registry_updates(*lists2, cur2, fin2, case["c"])
        assert summary2[1] == 0 and summary2[2] == 10 and summary2[5] == 13
        assert list(RU.process_registry_updates(vt, cur2, fin2, k)) == summary2
        LT.apply_update(items, range(n), 80, 32, [b"".join(int(x).to_bytes(8, "little") for x in row) for row in values2])
        assert vt.root() == LT.Model(LT.VALIDATOR, items).root(True)
    # a wrapped epoch raises after the tree is updated
    wrap = C.overflow_cases()[2]
    with state_tree.validator_registry_tree(64) as vt:
        rec = records(wrap)
        rec[:, 112] = 0
        vt.append([rec[i].tobytes() for i in range(wrap["n"])])
        with pytest.raises(OverflowError):
            RU.process_registry_updates(vt, wrap["cur"], wrap["fin"], constants(RU, wrap))
