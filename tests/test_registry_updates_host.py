"""The registry updates on the CPU: registry_updates_model.py against
tests/golden/registry_updates.json (the reference's spec text, make_registry_updates_vectors.py),
then the code the kernels share (csrc/bls381_regupd.hpp, host build) against the model and the
golden file, and the same header in a stand-alone ASan/UBSan program.  GPU half:
test_registry_updates_gpu.py."""
import ctypes
import hashlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import registry_updates_cases as C
import registry_updates_model as M

vp, u64, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_size_t
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "registry_updates.json")
OUT_FIELDS = ("activation_eligibility_epoch", "activation_epoch", "exit_epoch", "withdrawable_epoch")


@pytest.fixture(scope="module")
def L():
    import build_native
    lib = ctypes.CDLL(os.environ.get("BLS381_HOSTCHECK_LIB") or build_native.build_hostcheck())
    lib.hc_registry_updates.argtypes = [u64, vp, vp, vp, vp, vp, sz, u64, u64, vp, vp, vp, vp]
    lib.hc_registry_updates.restype = ctypes.c_int
    lib.hc_registry_updates_threads.argtypes = [u64, vp, vp, vp, vp, vp, sz, u64, u64, vp, ctypes.c_uint32, vp, vp, vp]
    lib.hc_registry_updates_threads.restype = ctypes.c_int
    lib.hc_exit_queue.argtypes = [u64, vp, vp, sz, u64, vp, vp]
    lib.hc_exit_queue.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def golden():
    """The stored states, the digested ones with their inputs rebuilt and checked against the digests."""
    fx = json.load(open(GOLDEN))
    maker = C.golden_maker()
    states = []
    for s in fx["states"]:
        c = dict(s["constants"])
        inputs = s["inputs"]
        if s["n"] >= fx["digest_from"]:
            rebuilt = maker.lists(maker.registry(s["seed"], s["n"], c))
            for f, digest in inputs.items():
                assert digest_of(rebuilt[f]) == digest, (s["preset"], s["n"], f)
            inputs = rebuilt
        states.append(dict(s, inputs=inputs, c=c, cur=fx["epoch"], fin=fx["finalized_epoch"]))
    return states


def digest_of(values):
    return hashlib.sha256(struct.pack("<%dQ" % len(values), *[int(v) for v in values])).hexdigest()


def p(a, off=0):
    return ctypes.c_void_p(a.ctypes.data + off)


def records(case):
    """The five fields in 121-byte records (other bytes 0xA5), exactly 121 n bytes."""
    n = len(case["eff"])
    rec = np.full((max(n, 1), 121), 0xA5, dtype=np.uint8)
    for f, off in zip(C.FIELDS, (80, 88, 96, 104, 113)):
        if n:
            rec[:n, off:off + 8] = np.ascontiguousarray(case[f], dtype="<u8").view(np.uint8).reshape(n, 8)
    return rec


def hc_updates(L, case, stride=8, threads=None):
    n = len(case["eff"])
    k = np.array(M.constants6(case["c"]), dtype=np.uint64)
    idx, val, summary = np.full(n + 1, 0x5A5A5A5A, np.uint32), np.zeros(4 * n + 1, np.uint64), np.zeros(8, np.uint64)
    if stride == 8:
        cols = [np.append(np.asarray(case[f], dtype=np.uint64), np.uint64(0)) for f in C.FIELDS]
        ptrs = [p(a) for a in cols]
    else:
        rec = records(case)
        ptrs = [p(rec, off) for off in (80, 88, 96, 104, 113)]
    if threads is None:
        rc = L.hc_registry_updates(n, *ptrs, stride, case["cur"], case["fin"], p(k), p(idx), p(val), p(summary))
    else:
        rc = L.hc_registry_updates_threads(n, *ptrs, stride, case["cur"], case["fin"], p(k), threads, p(idx), p(val), p(summary))
    return rc, [int(x) for x in idx[:n]], [[int(x) for x in row] for row in val[:4 * n].reshape(n, 4)], [int(x) for x in summary]


def as_case(state):
    ins = state["inputs"]
    return {"elig": ins["activation_eligibility_epoch"], "act": ins["activation_epoch"], "ext": ins["exit_epoch"],
            "wd": ins["withdrawable_epoch"], "eff": ins["effective_balance"], "cur": state["cur"], "fin": state["fin"],
            "c": state["c"]}


def check_outputs(state, values):
    for x, f in enumerate(OUT_FIELDS):
        got = [row[x] for row in values]
        want = state["outputs"][f]
        assert (digest_of(got) if isinstance(want, str) else got) == want, (state["preset"], state["overrides"], state["n"], f)


def test_model_matches_spec_text(golden):
    """The restatement gives what the reference's own text gave, field by field, in every state;
    the override states run with a churn limit above the minimum."""
    assert max(s["churn_limit"] for s in golden) > 4
    for s in golden:
        case = as_case(s)
        idx, values, summary = M.registry_updates(case["elig"], case["act"], case["ext"], case["wd"], case["eff"], s["cur"],
                                                  s["fin"], s["c"])
        check_outputs(s, values)
        assert summary[5] == s["churn_limit"] and summary[7] == 0
        assert summary[1] > 0 or s["n"] < 64


def test_model_exit_queue_matches_spec_text(golden):
    """ExitQueue-style arithmetic over the model's exit_queue() reproduces repeated initiate_validator_exit."""
    for s in golden:
        case = as_case(s)
        e0, c0, limit, _ = M.exit_queue(case["act"], case["ext"], s["cur"], s["c"])
        delay = s["c"]["MIN_VALIDATOR_WITHDRAWABILITY_DELAY"]
        for k, (_, ex, wd) in enumerate(s["exits"]):
            want = e0 + (min(c0, limit) + k) // limit
            assert (ex, wd) == (want, want + delay), (s["n"], k)


def test_host_build_matches_spec_text(L, golden):
    for s in golden:
        for stride in (8, 121):
            rc, idx, values, summary = hc_updates(L, as_case(s), stride)
            assert rc == 0
            check_outputs(s, values)
            assert summary[5] == s["churn_limit"]


@pytest.mark.parametrize("stride", [8, 121])
def test_host_build_matches_model(L, stride):
    for case in C.all_accepted_cases() + C.random_cases(400):
        want = case.expected()
        assert want is not None, case["name"]
        rc, idx, values, summary = hc_updates(L, case, stride)
        assert rc == 0, case["name"]
        assert idx == want[0], case["name"]
        assert values == want[1], case["name"]
        assert summary == want[2], case["name"]


def test_host_build_on_threads_matches_model(L):
    """Slices of the registry on a thread each: 16 (more slices than validators in the small cases)
    and 5 (slices that do not divide n) give what one thread gives."""
    for case in C.all_accepted_cases() + C.random_cases(60, seed=2):
        want = case.expected()
        for threads in (16, 5):
            rc, idx, values, summary = hc_updates(L, case, 8, threads)
            assert rc == 0 and summary == want[2], case["name"]
            assert idx == want[0] and values == want[1], case["name"]
    assert hc_updates(L, C.Case("too many threads", 8), 8, 65)[0] != 0


def test_cases_are_what_their_names_say():
    by = {c["name"]: c for c in C.all_accepted_cases()}
    assert by["L=12 with quotient 16"].expected()[2][5] == 12
    big = by["L above 256"].expected()[2]
    assert big[5] == 341 and big[1] == 342
    assert by["one wrapping exit_epoch"].expected()[2][7] == 1
    assert by["exit epochs at and past 2^64 - 1"].expected()[2][7] == 6
    assert by["a withdrawable_epoch that wraps alone"].expected()[2][7] == 1
    assert by["L >= K with quotient 1"].expected()[2][2] == len(range(0, 300, 7))
    got = by["equal keys across the threshold, two tiles"].expected()
    assert [i for i in got[0] if i != M.NONE] == [2045, 2046, 2047, 2048]
    assert all(c.expected() is None for c in C.rejected_cases())


def test_host_build_second_scan_round(L):
    case = C.second_scan_round_case()
    want = case.expected()
    n = case["n"]
    assert want[2][5] == 7 and want[2][1] == 4 and want[2][2] == 6          # L, ejected, activated
    assert want[0][n - 1] == n - 1 and want[1][n - 1][1] == C.DELAYED_FIN    # tile 256: ejected, in the queue
    assert want[0][100] == M.NONE                                            # the place it takes
    for threads in (None, 16):
        rc, idx, values, summary = hc_updates(L, case, 8, threads)
        assert rc == 0 and summary == want[2]
        assert idx == want[0] and values == want[1]


def test_host_build_rejects(L):
    for case in C.rejected_cases():
        assert hc_updates(L, case)[0] != 0, case["name"]


def test_host_exit_queue(L, golden):
    cases = [as_case(s) for s in golden] + C.exit_queue_cases() + C.random_cases(100, seed=5)
    for case in cases:
        act, ext = (np.append(np.asarray(case[f], dtype=np.uint64), np.uint64(0)) for f in ("act", "ext"))
        k, q = np.array(M.constants6(case["c"]), dtype=np.uint64), np.zeros(4, np.uint64)
        assert L.hc_exit_queue(len(act) - 1, p(act), p(ext), 8, case["cur"], p(k), p(q)) == 0
        assert [int(x) for x in q] == list(M.exit_queue([int(x) for x in case["act"]], [int(x) for x in case["ext"]],
                                                       case["cur"], case["c"]))


def text(*items):
    out = []
    for it in items:
        if isinstance(it, (list, tuple, np.ndarray)):
            for x in it:
                out.append(text(x) if isinstance(x, (list, tuple)) else str(int(x)))
        else:
            out.append(str(int(it)))
    return " ".join(out)


def test_standalone_program_under_sanitizers(golden, tmp_path):
    """The same header behind its own main, built with -fsanitize=address,undefined, over buffers of
    exactly the bytes the fields span.  Nothing loaded into Python runs under a sanitizer."""
    import build_native
    exe = build_native.build_regupd_check()
    lines = []
    cases = [c for c in C.all_accepted_cases() if c["n"] <= 4097] + C.random_cases(60, seed=9) + C.rejected_cases()
    for case in cases:
        want = case.expected()
        for stride in (8, 121):
            head = text(case["n"], stride, case["cur"], case["fin"], M.constants6(case["c"]), *case.lists())
            lines.append("R " + head + (" 1" if want is None else " 0 " + text(*want)))
    for case in C.exit_queue_cases():
        act, ext = case.lists()[1:3]
        for stride in (8, 121):
            lines.append("Q " + text(case["n"], stride, case["cur"], M.constants6(case["c"]), act, ext, 0,
                                     M.exit_queue(act, ext, case["cur"], case["c"])))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    run = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.split()[:4] == [str(len(lines)), "cases,", "0", "mismatches"], run.stdout


def test_exit_queue_object_without_a_device(golden):
    """ExitQueue.initiate() is arithmetic alone: over the model's view of each golden state it gives
    the spec text's sequence, and an epoch past 2^64 - 1 raises and leaves the queue where it was."""
    from bls381_amd.registry_updates import ExitQueue
    for s in golden:
        case = as_case(s)
        q = ExitQueue(*M.exit_queue(case["act"], case["ext"], s["cur"], s["c"]), s["c"]["MIN_VALIDATOR_WITHDRAWABILITY_DELAY"])
        assert [q.initiate() for _ in s["exits"]] == [(ex, wd) for _, ex, wd in s["exits"]]
    q = ExitQueue(M.FAR - 257, 3, 4, 100, 256)
    assert q.initiate() == (M.FAR - 257, M.FAR - 1)
    with pytest.raises(OverflowError):      # the next exit moves on to FAR - 256, whose withdrawable epoch is FAR: allowed
        q.initiate(), q.initiate(), q.initiate(), q.initiate(), q.initiate()
    assert (q.epoch, q.churn) == (M.FAR - 256, 4)
    with pytest.raises(OverflowError):
        q.initiate()
    assert (q.epoch, q.churn) == (M.FAR - 256, 4)
    with pytest.raises(ValueError):
        ExitQueue(10, 0, 0, 0, 256)
