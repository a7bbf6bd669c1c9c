"""Host planners of the launch pipelines (consensus-specs_amd/csrc/bls381_plan.hpp), CPU only.

The planners hold py_ecc's grouping semantics and every workspace byte count; they contain no
HIP call, and libbls381_hostcheck.so (test infrastructure, host_check.cpp) exports them as flat
arrays.  These tests pin what the GPU tests imply.
"""
import ctypes
import os
from collections import Counter

import pytest

PAIR_NONE = -(1 << 31)
KBLOCK = 128
PROD_CHUNK = 8
BLS_VM_TASK_MAX = 8192
SSZ_CHUNK, SSZ_MERKLE, SSZ_STACK = 1, 2, 64
INF48 = b"\xc0" + bytes(47)
INF96 = b"\xc0" + bytes(95)
CAP = 1 << 21   # u32 words of a dump buffer


@pytest.fixture(scope="module")
def L():
    import build_native
    lib = ctypes.CDLL(os.environ.get("BLS381_HOSTCHECK_LIB") or build_native.build_hostcheck())
    for f in (lib.hc_plan_products, lib.hc_plan_agg, lib.hc_plan_vm, lib.hc_plan_vm_grouped):
        f.restype = ctypes.c_long
    lib.hc_vm_ws_bounds.restype = None
    lib.hc_deposit_prog.restype = ctypes.c_uint32
    return lib


def u32s(v): return (ctypes.c_uint32 * max(1, len(v)))(*v)
def sz(x): return ctypes.c_size_t(x)


class Reader:
    def __init__(self, words): self.w, self.i = words, 0
    def u(self):
        self.i += 1
        return self.w[self.i - 1]
    def vec(self, signed=False):
        v = [self.u() for _ in range(self.u())]
        return [x - (1 << 32) if x >= 1 << 31 else x for x in v] if signed else v
    def lists(self):
        return [[(self.u(), self.u()) for _ in range(self.u())] for _ in range(self.u())]


def dump(call, *args):
    out = (ctypes.c_uint32 * CAP)()
    n = call(*args, out, sz(CAP))
    assert n >= 0
    return list(out[:n])


def fold(passes, n_in):
    """The passes over the multisets {0}, {1}, ...: what each final value is a product of."""
    vals = [Counter([i]) for i in range(n_in)]
    for p in passes:
        assert all(e - b <= PROD_CHUNK for b, e in p)
        vals = [sum((vals[i] for i in range(b, e)), Counter()) for b, e in p]
    return vals


# ------------------------------------------------------------ plan_products
@pytest.mark.parametrize("off", [[0, 1], [0, 8], [0, 9], [0, 64], [0, 65], [0, 0], [0, 9, 9, 80, 81]])
def test_plan_products(L, off):
    r = Reader(dump(L.hc_plan_products, sz(len(off) - 1), u32s(off)))
    passes = r.lists()
    assert len(passes) >= 1
    vals = fold(passes, off[-1])
    assert len(vals) == len(off) - 1                       # every segment ends as one value
    for c, v in enumerate(vals):                           # holding each of its inputs exactly once
        assert v == Counter(range(off[c], off[c + 1]))
    if off == [0, 0]:
        assert passes == [[(0, 0)]]                        # an empty segment: one empty chunk


# ----------------------------------------------------------------- plan_agg
def check_level(chunks, off):
    """Chunks cover each group's range [off[g], off[g+1]) once, in order; returns the next offsets."""
    nxt, k = [0], 0
    for g in range(len(off) - 1):
        b, e = off[g], off[g + 1]
        if e == b:
            assert chunks[k] == (b, b)
            k += 1
        else:
            at = b
            while at < e:
                assert chunks[k][0] == at and at < chunks[k][1] <= e
                at = chunks[k][1]
                k += 1
        nxt.append(k)
    assert k == len(chunks)
    return nxt


@pytest.mark.parametrize("lanes", [1, 2])
def test_plan_agg(L, lanes):
    pr = KBLOCK // lanes
    for sizes in ([0, 1, pr - 1, pr, pr + 1, 4 * pr + 1], [1 << 17], [0], [0, 0, 5]):
        off = [0]
        for s in sizes:
            off.append(off[-1] + s)
        ws = (ctypes.c_size_t * 2)()
        # 3 Fp components per point: the public bound is the G1 one (its chunk count holds for both widths)
        out = (ctypes.c_uint32 * CAP)()
        n = L.hc_plan_agg(sz(len(sizes)), u32s(off), lanes, 3, out, sz(CAP), ws)
        assert n >= 0
        levels = Reader(list(out[:n])).lists()
        cur = off
        for lv in levels:
            cur = check_level(lv, cur)                     # level 0 covers the ranges, later ones the chunks below
        assert len(levels[-1]) == len(sizes)               # one chunk per group
        assert all(len(lv) > len(sizes) for lv in levels[:-1])
        assert ws[0] <= ws[1]


# ------------------------------------------------------------------ plan_vm
def parse_vm(words):
    r = Reader(words)
    p = dict(zip(("n_calls", "n_keys", "G", "nquads", "tasks", "nslots"), (r.u() for _ in range(6))))
    p["ws_bound"] = r.u() | (r.u() << 32)
    p["key_idx"], p["group_off"], p["group_msg"], p["group_call"] = r.vec(), r.vec(), bytes(r.vec()), r.vec()
    p["quad_pair"], p["call_quad_off"] = r.vec(signed=True), r.vec()
    p["passes"], p["task_passes"] = r.lists(), r.lists()
    p["quad_slot"], p["sig_slot"], p["sig_task"] = r.vec(), r.vec(), r.vec(signed=True)
    p["agg"] = r.lists()
    assert r.i == len(words)
    return p


def plan_vm(L, calls, mlen, with_sig=None, host=True):
    """calls: [(keys, msgs, sig)]; host: the key / signature bytes are given to the planner."""
    off, keys, msgs = [0], b"", b""
    for k, m, _ in calls:
        off.append(off[-1] + len(k))
        keys += b"".join(k)
        msgs += b"".join(m)
    sigs = b"".join(s for _, _, s in calls)
    ws = (ctypes.c_int * max(1, len(calls)))(*(with_sig or [1] * len(calls)))
    words = dump(L.hc_plan_vm, sz(len(calls)), u32s(off), msgs, sz(mlen), keys if host else None,
                 sigs if host else None, ws)
    return parse_vm(words)


def model_vm(calls, with_sig=None):
    """py_ecc's verify_multiple grouping: distinct messages in first-occurrence order, members in
    index order; an all-infinite group and an infinite signature are dropped; no pairs: one idle quad."""
    groups, quad_pair, cqo, base = [], [], [0], 0
    for c, (keys, msgs, sig) in enumerate(calls):
        order = {}
        for i, m in enumerate(msgs):
            order.setdefault(m, []).append(base + i)
        pairs = []
        for m, idx in order.items():
            if all(keys[i - base] == INF48 for i in idx):
                continue
            pairs.append(len(groups))
            groups.append((c, m, idx))
        if (with_sig is None or with_sig[c]) and sig != INF96:
            pairs.append(-(c + 1))
        pairs = pairs or [PAIR_NONE]
        quad_pair += pairs + [PAIR_NONE] * (len(pairs) % 2)
        cqo.append(len(quad_pair) // 2)
        base += len(keys)
    return groups, quad_pair, cqo


def key(i): return bytes([0x80 | (i % 31), i % 251]) + bytes(46)
def msg(i, mlen): return bytes([i + 1]) * mlen
SIG = b"\x8f" + bytes(95)


def small_batches(mlen):
    m = lambda i: msg(i, mlen)
    return [
        [([], [], SIG)],
        [([key(0)], [m(0)], SIG)],
        [([key(0), key(1)], [m(0), m(0)], SIG), ([key(2), key(3)], [m(0), m(1)], SIG)],
        [([key(0), key(1), key(2)], [m(0), m(1), m(0)], SIG), ([], [], INF96)],
        [([key(i) for i in range(5)], [m(2), m(0), m(2), m(1), m(0)], SIG),
         ([INF48, key(1), INF48], [m(0), m(1), m(0)], SIG),                     # group m(0) all-infinite: dropped
         ([INF48], [m(3)], INF96),                                              # nothing left: PAIR_NONE
         ([INF48, key(7)], [m(1), m(1)], INF96)],
    ]


@pytest.mark.parametrize("mlen", [0, 32])
def test_plan_vm_small(L, mlen):
    for calls in small_batches(mlen):
        p = plan_vm(L, calls, mlen)
        groups, quad_pair, cqo = model_vm(calls)
        assert p["tasks"] == 1 and p["n_calls"] == len(calls) and p["G"] == len(groups)
        assert p["key_idx"] == [i for _, _, idx in groups for i in idx]
        assert p["group_off"] == [0] + [sum(len(g[2]) for g in groups[:k + 1]) for k in range(len(groups))]
        assert p["group_msg"] == b"".join(m for _, m, _ in groups)
        assert p["group_call"] == [c for c, _, _ in groups]
        assert p["quad_pair"] == quad_pair and p["call_quad_off"] == cqo and p["nquads"] == cqo[-1]
        vals = fold(p["task_passes"], 2 * p["nquads"])       # one value per call: its pair tasks, once each
        assert vals == [Counter(range(2 * cqo[c], 2 * cqo[c + 1])) for c in range(len(calls))]
        nk = sum(len(k) for k, _, _ in calls)
        bounds = (ctypes.c_size_t * 3)()
        L.hc_vm_ws_bounds(sz(len(calls)), sz(nk), sz(mlen), sz(1), bounds)
        assert bounds[0] >= p["ws_bound"]


def test_plan_vm_with_sig_and_device_keys(L):
    calls = [([INF48, key(1)], [msg(0, 32), msg(0, 32)], SIG), ([INF48], [msg(1, 32)], INF96)]
    p = plan_vm(L, calls, 32, with_sig=[0, 1])
    assert p["quad_pair"] == model_vm(calls, [0, 1])[1] == [0, PAIR_NONE, PAIR_NONE, PAIR_NONE]
    # device-resident keys and signatures: nothing is dropped
    p = plan_vm(L, calls, 32, host=False)
    assert p["quad_pair"] == [0, -1, 1, -2] and p["key_idx"] == [0, 1, 2]


def test_plan_vm_large(L):
    n_calls, mlen = 4200, 32
    calls = [([key(2 * c), key(2 * c + 1)], [msg(0, mlen), msg(1, mlen)], SIG) for c in range(n_calls)]
    p = plan_vm(L, calls, mlen)
    assert 2 * 2 * n_calls > BLS_VM_TASK_MAX and p["tasks"] == 0   # three pairs, two quads per call
    assert p["G"] == 2 * n_calls and p["key_idx"] == list(range(2 * n_calls))
    halves = [v for v in p["quad_pair"] if v != PAIR_NONE]
    assert sorted(halves) == list(range(p["G"]))                   # every group in exactly one quad half
    assert p["sig_task"] == [-(c + 1) for c in range(n_calls)]
    assert p["nslots"] == p["nquads"] + n_calls
    assert sorted(p["quad_slot"] + p["sig_slot"]) == list(range(p["nslots"]))
    vals = fold(p["passes"], p["nslots"])
    cqo = p["call_quad_off"]
    assert vals == [Counter([p["quad_slot"][q] for q in range(cqo[c], cqo[c + 1])] + [p["sig_slot"][c]])
                    for c in range(n_calls)]
    for c in range(n_calls):                                       # a quad's groups belong to its call
        for q in range(cqo[c], cqo[c + 1]):
            assert all(v == PAIR_NONE or p["group_call"][v] == c for v in p["quad_pair"][2 * q:2 * q + 2])
    bounds = (ctypes.c_size_t * 3)()
    L.hc_vm_ws_bounds(sz(n_calls), sz(2 * n_calls), sz(mlen), sz(1), bounds)
    assert bounds[0] >= p["ws_bound"]


# ---------------------------------------------------------- plan_vm_grouped
@pytest.mark.parametrize("mlen", [0, 32])
def test_plan_vm_grouped(L, mlen):
    m = lambda i: msg(i, mlen)
    # per call: [(message, number of keys)]; equal messages merge, empty groups drop
    batch = [[(m(0), 2), (m(1), 0), (m(0), 1), (m(2), 3)], [], [(m(1), 0)], [(m(3), 1), (m(3), 1), (m(0), 2)]]
    cgo, gko, gmsgs, calls, k = [0], [0], b"", [], 0
    for groups in batch:
        keys, msgs = [], []
        for gm, cnt in groups:
            gko.append(gko[-1] + cnt)
            gmsgs += gm
            keys += [key(k + j) for j in range(cnt)]
            msgs += [gm] * cnt
            k += cnt
        cgo.append(cgo[-1] + len(groups))
        calls.append((keys, msgs, SIG))
    g = parse_vm(dump(L.hc_plan_vm_grouped, sz(len(batch)), u32s(cgo), u32s(gko), gmsgs, sz(mlen)))
    flat = plan_vm(L, calls, mlen, host=False)
    assert g == flat
    if mlen:
        assert g["key_idx"][:3] == [0, 1, 2] and g["group_off"][:3] == [0, 3, 6]   # m(0): groups 0 and 2 merged
    bounds = (ctypes.c_size_t * 3)()
    L.hc_vm_ws_bounds(sz(len(batch)), sz(k), sz(mlen), sz(1), bounds)
    assert bounds[0] >= g["ws_bound"]


# --------------------------------------------------------- workspace bounds
@pytest.mark.parametrize("n", [1, 2, 8192, 8193, 49152, 49153, 65537])
def test_verify_ws_size_covers_its_carve(L, n):
    bounds = (ctypes.c_size_t * 3)()
    L.hc_vm_ws_bounds(sz(1), sz(1), sz(32), sz(n), bounds)
    assert bounds[1] >= bounds[2] > 0


# -------------------------------------------------------------- ssz_prog_ok
def test_ssz_prog_ok(L):
    ok = lambda prog, item: L.hc_ssz_prog_ok(u32s(prog), len(prog), sz(item))
    buf, item = (ctypes.c_uint32 * 512)(), ctypes.c_size_t()
    plen = L.hc_deposit_prog(buf, ctypes.byref(item))
    deposit = list(buf[:plen])
    assert item.value == 184 and ok(deposit, 184)
    assert not ok(deposit, 87)                                            # the amount chunk reaches past the item
    assert ok([SSZ_CHUNK, 176, 8], 184) and not ok([SSZ_CHUNK, 180, 8], 184)
    assert not ok([SSZ_CHUNK, 0, 33], 184)
    assert not ok([SSZ_CHUNK, 0, 32, SSZ_CHUNK, 32, 32], 184)             # unbalanced stack
    assert not ok([SSZ_CHUNK, 0, 32, SSZ_MERKLE, 2], 184)                 # pops more than it holds
    assert not ok([SSZ_CHUNK, 0, 32, SSZ_MERKLE, 0], 184)                 # k = 0
    assert not ok([SSZ_CHUNK, 0], 184) and not ok([SSZ_CHUNK, 0, 32, SSZ_MERKLE], 184)   # truncated
    assert not ok([], 184) and not ok([3, 0, 32], 184)
    chunks = lambda k: [SSZ_CHUNK, 0, 32] * k + [SSZ_MERKLE, k]
    assert ok(chunks(SSZ_STACK), 32) and not ok(chunks(SSZ_STACK + 1), 32)          # peak above SSZ_STACK
    assert ok(chunks(33), 32) and not ok([SSZ_CHUNK, 0, 32] + chunks(33) + [SSZ_MERKLE, 2], 32)   # padded to 64 above one
