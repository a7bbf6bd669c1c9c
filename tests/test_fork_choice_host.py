"""The fork choice on the CPU: fork_choice_model.py against tests/golden/fork_choice.json (the
reference's spec text, make_fork_choice_vectors.py), then the code the kernels share
(csrc/bls381_forkchoice.hpp, host build) against the model over the crafted cases, and the same
header in a stand-alone ASan/UBSan program.  GPU half: test_fork_choice_gpu.py."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import fork_choice_cases as C
import fork_choice_model as M

vp, u64, u32, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_size_t
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fork_choice.json")
RECORD, OFFSETS = 121, (88, 96, 113)


@pytest.fixture(scope="module")
def L():
    import build_native
    lib = ctypes.CDLL(os.environ.get("BLS381_HOSTCHECK_LIB") or build_native.build_hostcheck())
    for name, res, args in (
            ("create", vp, [u64, u64]), ("destroy", None, [vp]), ("block_count", u64, [vp]),
            ("add_blocks", ctypes.c_int, [vp, u64, vp, vp, vp, vp]), ("node", u32, [vp, vp]),
            ("on_attestations", ctypes.c_int, [vp, u64, vp, vp, vp, vp, vp, vp]),
            ("read_latest", ctypes.c_int, [vp, u64, u64, vp, vp]), ("prune", ctypes.c_int, [vp, u32]),
            ("head", ctypes.c_int, [vp, u32, u64, vp, vp, vp, sz, u64, vp, vp, vp, vp])):
        fn = getattr(lib, "hc_fork_choice_" + name)
        fn.restype, fn.argtypes = res, args
    return lib


@pytest.fixture(scope="module")
def golden():
    """The stored scenarios with their inputs rebuilt from the seeds and checked against what is stored."""
    fx = json.load(open(GOLDEN))
    maker = C.golden_maker()
    out = []
    for s in fx["scenarios"]:
        sc = maker.scenario(s["seed"], s["n"], s["kind"])
        full = s["n"] < fx["digest_from"]
        assert maker.blocks_digest(sc["blocks"]) == s["blocks"] and len(sc["blocks"]) == s["n_blocks"]
        for name, words in (("validators", maker.validator_words(sc["validators"])), ("log", maker.log_words(sc["log"]))):
            assert (words if full else maker.digest(words)) == s[name], (s["kind"], s["n"], name)
        out.append((s, sc, maker))
    return out


def p(a, off=0):
    return ctypes.c_void_p(a.ctypes.data + off)


def arr(values, dtype):
    """One spare entry, so no array is empty."""
    a = np.zeros(len(values) + 1, dtype)
    a[:len(values)] = np.asarray([int(x) for x in values], dtype=dtype) if len(values) else []
    return a


def roots_arr(roots):
    return np.frombuffer(b"".join(bytes(r) for r in roots) + bytes(32), dtype=np.uint8).copy()


def fields(act, ext, eff, stride):
    """Pointers to the three fields: plain arrays, or 121-byte records (other bytes 0xA5)."""
    n = len(eff)
    if stride == 8:
        cols = [arr(x, np.uint64) for x in (act, ext, eff)]
        return cols, [p(c) for c in cols]
    rec = np.full((max(n, 1), RECORD), 0xA5, dtype=np.uint8)
    for col, off in zip((act, ext, eff), OFFSETS):
        if n:
            rec[:n, off:off + 8] = np.asarray([int(x) for x in col], dtype="<u8").view(np.uint8).reshape(n, 8)
    return [rec], [p(rec, off) for off in OFFSETS]


class HostBackend:
    """The calls of a script on the host build."""

    def __init__(self, lib, stride=8):
        self.L, self.stride, self.fc = lib, stride, None

    def close(self):
        self.L.hc_fork_choice_destroy(self.fc)
        self.fc = None

    def create(self, vcap, bcap):
        self.close()
        self.fc = self.L.hc_fork_choice_create(vcap, bcap)
        assert self.fc

    def add_blocks(self, roots, parents, slots):
        n = len(roots)
        r, pr, s, ids = roots_arr(roots), roots_arr(parents), arr(slots, np.uint64), np.full(n + 1, 0x5A5A5A5A, np.uint32)
        if self.L.hc_fork_choice_add_blocks(self.fc, n, p(r), p(pr), p(s), p(ids)):
            assert all(ids == 0x5A5A5A5A)
            return None
        assert [self.L.hc_fork_choice_node(self.fc, p(r, 32 * k)) for k in range(n)] == [int(x) for x in ids[:n]]
        return [int(x) for x in ids[:n]]

    def on_attestations(self, att_off, entries, slots, targets, ok):
        n_att = len(slots)
        o, e, s, t = arr(att_off, np.uint32), arr(entries, np.uint32), arr(slots, np.uint64), arr(targets, np.uint32)
        k = arr(ok, np.uint8) if ok is not None else None
        skipped = np.full(1, 0x5A5A, np.uint64)
        if self.L.hc_fork_choice_on_attestations(self.fc, n_att, p(o), p(e), p(s), p(t), p(k) if ok is not None else None,
                                                 p(skipped)):
            assert skipped[0] == 0x5A5A
            return None
        return int(skipped[0])

    def latest(self, first, n):
        slots, targets = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint32)
        if self.L.hc_fork_choice_read_latest(self.fc, first, n, p(slots), p(targets)):
            return None
        return [int(x) for x in slots[:n]], [int(x) for x in targets[:n]]

    def prune(self, node):
        return None if self.L.hc_fork_choice_prune(self.fc, node) else True

    def head(self, start, act, ext, eff, epoch):
        B = int(self.L.hc_fork_choice_block_count(self.fc))
        keep, ptrs = fields(act, ext, eff, self.stride)
        head, root = np.full(1, 0x5A5A5A5A, np.uint32), np.zeros(32, np.uint8)
        weights, status = np.full(B + 1, 0x5A, np.uint64), np.full(1, 0x5A, np.uint64)
        if self.L.hc_fork_choice_head(self.fc, start, len(eff), *ptrs, self.stride, epoch, p(head), p(root), p(weights), p(status)):
            assert head[0] == 0x5A5A5A5A and all(weights == 0x5A) and status[0] == 0x5A
            return None
        assert weights[B] == 0x5A
        return int(head[0]), bytes(root), [int(x) for x in weights[:B]], int(status[0])


def run_host(L, script, stride=8):
    b = HostBackend(L, stride)
    try:
        return C.run_script(script, b)
    finally:
        b.close()


# ---- the model against the spec text -------------------------------------------------------------------------------
def test_model_matches_spec_text(golden):
    """The restatement gives what the reference's own text gave in every scenario: the head, every
    block's vote count and every validator's latest message."""
    for s, sc, maker in golden:
        res = C.expected(C.golden_script(sc))
        slots, targets = res[3]
        head, root, counts, status = res[4]
        full = isinstance(s["latest_slot"], list)
        assert (slots if full else maker.digest(slots)) == s["latest_slot"], (s["kind"], s["n"])
        assert (targets if full else maker.digest(targets)) == s["latest_target"], (s["kind"], s["n"])
        assert (head, root.hex(), counts, status) == (s["head"], s["head_root"], s["vote_counts"], 0), (s["kind"], s["n"])


def test_golden_scenarios_are_what_their_names_say(golden):
    for s, sc, maker in golden:
        counts, blocks = s["vote_counts"], sc["blocks"]
        kids = [i for i, b in enumerate(blocks) if b[1] == s["start"]]
        if s["kind"] == "tie":
            assert counts[kids[0]] == counts[kids[1]]                       # the root decided
        if s["kind"] == "heavy_second" and s["n"] >= 7:
            direct_first = counts[kids[0]]                                  # a leaf: all of it is direct
            assert counts[kids[1]] > direct_first and blocks[s["head"]][1] != 0
        if s["kind"] == "outside":
            assert s["start"] > 0 and counts[0] >= counts[s["start"]]
            assert s["n"] < 64 or counts[0] > counts[s["start"]]            # votes above and beside the start block
    mixed = [sc for s, sc, _ in golden if s["kind"] == "mixed" and s["n"] >= 64]
    for sc in mixed:
        seen = {}
        for slot, _, members in sc["log"]:
            for i in members:
                seen.setdefault(i, []).append(slot)
        assert any(len(v) > len(set(v)) for v in seen.values())            # equal slots for one validator
        assert len(seen) < len(sc["validators"])                           # validators without a message
        assert any(v.effective_balance == 0 for v in sc["validators"])


# ---- the host build against the model ------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [8, 121])
def test_host_build_matches_spec_text(L, golden, stride):
    for s, sc, maker in golden:
        res = run_host(L, C.golden_script(sc), stride)
        assert res[4] == (s["head"], bytes.fromhex(s["head_root"]), s["vote_counts"], 0), (s["kind"], s["n"])
        assert res == C.expected(C.golden_script(sc))


@pytest.mark.parametrize("stride", [8, 121])
def test_host_build_matches_model(L, stride):
    for name, script in C.small_cases().items():
        assert run_host(L, script, stride) == C.expected(script), name
    for k, script in enumerate(C.random_scripts(150)):
        assert run_host(L, script, stride) == C.expected(script), k


def test_host_build_at_the_kernels_bounds(L):
    for cases in (C.validator_size_cases(), C.block_size_cases()):
        for name, script in cases.items():
            assert run_host(L, script) == C.expected(script), name


def test_cases_are_what_their_names_say():
    by = C.small_cases()
    for name, script in C.rejected_cases().items():
        res = C.expected(script)
        assert res[3] is None, name                                  # the fourth call is the rejected one
        accepted = C.expected(script[:3] + script[4:])
        assert res[4:] == accepted[3:], name                         # and it changed nothing
    head, root, counts, status = C.expected(by["a sum that wraps"])[-1]
    assert status == 3 and counts == [M.MAX64, M.MAX64, M.MAX64, 2 ** 63]   # 2^64 at the tip, more above it
    head, root, counts, status = C.expected(by["sums at the edge"])[-1]
    assert status == 2 and counts == [M.MAX64, M.MAX64, M.MAX64, 2 ** 32 - 1]   # the tip holds 2^64 - 1 exactly: not counted
    for which in ("last", "first"):
        script = by["equal counts, roots differ in the %s byte" % which]
        head, root, counts, _ = C.expected(script)[-1]
        assert counts[1] == counts[2] == counts[3] and head == 2     # 0xF0 is the largest byte
    res = C.expected(by["two batches"])
    assert res[4][1][1:6] == [4, 4, 7, 5, 8]                         # the later batch lost at equal slots, won at a higher one
    res = C.expected(by["verdicts with failures"])
    assert res[2] == 0 and res[4][1][1:4] == [8, 6, 6]               # no message (target 5) from the failed one at slot 205
    res = C.expected(by["entries out of range"])
    assert res[2] == 4
    assert C.expected(by["every member on one validator"])[3][1][9] == 6
    chain = C.expected(C.block_size_cases()["a chain of 1025, no votes"])[-1]
    assert chain[0] == 1024


def test_prune_matches_fresh_store(L):
    """The head and counts after prune equal a fresh store fed the surviving blocks and the same log."""
    script, blocks, votes, reg, anchor = C.prune_cases()
    kept, new = C.surviving(blocks, anchor)
    assert 1 < len(kept) < len(blocks)
    tag, off, entries, slots, targets, ok = votes
    # the same log: attestations whose target went are handed in all the same (they take their seq)
    # with a verdict of 0, which leaves no message
    fresh = [("S", len(reg[0]), 30), C.add_call(kept),
             ("A", off, entries, slots, [new.get(t, 0) for t in targets], [t in new for t in targets]),
             ("H", 0) + reg + (C.EPOCH,)]
    for run in (C.expected, lambda s: run_host(L, s)):
        pruned, want = run(script), run(fresh)
        assert pruned[6] == want[3]
        latest_slots, latest_targets = pruned[5]
        assert [t for t in latest_targets if t != M.NONE] == [t for t in run(fresh + [("L", 0, len(reg[0]))])[4][1] if t != M.NONE]
        assert any(s and t == M.NONE for s, t in zip(latest_slots, latest_targets))   # a kept key without a target


# ---- the stand-alone program ----------------------------------------------------------------------------------------------
def text(*items):
    out = []
    for it in items:
        if isinstance(it, (bytes, bytearray)):
            out.extend(str(x) for x in it)
        elif isinstance(it, (list, tuple, np.ndarray)):
            out.append(text(*it))
        else:
            out.append(str(int(it)))
    return " ".join(x for x in out if x)


def script_text(script, stride):
    """The script with the model's results, in the program's format."""
    lines = []
    for call, want in zip(script, C.expected(script)):
        tag, a = call[0], call[1:]
        rc = " 1" if want is None else " 0 "
        if tag == "S":
            lines.append("S " + text(*a))
        elif tag == "B":
            lines.append("B " + text(len(a[0]), a[0], a[1], a[2]) + rc + ("" if want is None else text(want)))
        elif tag == "A":
            ok = a[4]
            lines.append("A " + text(len(a[2]), a[0], len(a[1]), a[1], a[2], a[3], ok is not None, ok if ok is not None else [])
                         + rc + ("" if want is None else text(want)))
        elif tag == "L":
            lines.append("L " + text(*a) + rc + ("" if want is None else text(*want)))
        elif tag == "P":
            lines.append("P " + text(*a) + rc.rstrip())
        else:
            start, act, ext, eff, epoch = a
            lines.append("H " + text(start, len(eff), stride, epoch, act, ext, eff) + rc +
                         ("" if want is None else text(want[0], want[1], len(want[2]), want[2], want[3])))
    return lines


def test_standalone_program_under_sanitizers(golden, tmp_path):
    """The same header behind its own main, built with -fsanitize=address,undefined, over buffers of
    exactly the bytes the arrays and fields span.  Nothing loaded into Python runs under a sanitizer."""
    import build_native
    exe = build_native.build_forkchoice_check()
    scripts = list(C.small_cases().values()) + C.random_scripts(60, seed=9) + [C.golden_script(sc) for _, sc, _ in golden]
    sized = C.block_size_cases()
    scripts += [sized[name] for name in ("256 blocks", "257 blocks", "a comb", "a chain of 1025")]
    scripts.append(C.validator_size_cases()["2049 validators"])
    lines = []
    for script in scripts:
        for stride in (8, 121):
            lines += script_text(script, stride)
    path = tmp_path / "script.txt"
    path.write_text("\n".join(lines) + "\n")
    run = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.split()[:4] == [str(len(lines)), "calls,", "0", "mismatches"], run.stdout
