"""Committee selection on the device: bls381_shuffle / bls381_attesting_entries and
their Python front (bls381_amd/committees.py) against tests/golden/shuffling.json and the spec
restated in shuffle_model.py, then shuffle -> attesting entries -> grouped registry verify on
device buffers.  CPU half: test_shuffle_host.py."""
import ctypes
import random

import numpy as np
import pytest

import shuffle_model as M

pytestmark = pytest.mark.gpu

ROUNDS = [10, 90]
SEED = M.generator_seeds()[0]
BIG = 65793                                  # 65,536 + 257: several workgroups, counter byte 2, a ragged last block
HUGE = 2 ** 32 - 1
ATT_LENGTHS = [0, 1, 9, 128, 257, 4096]


def cvp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def committees(native):
    from bls381_amd import committees
    return committees


@pytest.fixture(scope="module")
def lists():
    """The model's whole lists, computed once: {(n, rounds): uint32 array}."""
    return {(n, r): M.shuffled_list(n, SEED, r) for n in (1, 2, 3, 255, 256, 257, 1000, BIG) for r in ROUNDS}


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
        def u32(t):
            return np.frombuffer(t.cpu().numpy().tobytes(), dtype=np.uint32)

        @staticmethod
        def empty(nbytes, fill=0xEE):
            return torch.full((max(int(nbytes), 1),), fill, dtype=torch.uint8, device=Dev.device)

    return Dev


# ------------------------------------------------------------------- the shuffle
@pytest.mark.parametrize("rounds", ROUNDS)
@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 1000])
def test_full_list(committees, lists, n, rounds):
    got = committees.shuffled_indices(n, SEED, rounds)
    assert got.dtype == np.uint32 and np.array_equal(got, lists[(n, rounds)])
    for c in M.fixture()["cases"]:
        if (c["rounds"], c["seed"], c["count"]) == (rounds, 0, n):
            assert M.list_digest(got) == c["sha256"] and got.tolist() == c["shuffled"]


@pytest.mark.parametrize("rounds", ROUNDS)
def test_full_list_several_workgroups(committees, lists, rounds):
    got = committees.shuffled_indices(BIG, SEED, rounds)
    assert np.array_equal(got, lists[(BIG, rounds)])
    assert np.array_equal(np.sort(got), np.arange(BIG, dtype=np.uint32))


def test_every_generator_seed_at_1000(committees):
    """All 30 seeds of the reference's generator at its largest count, by digest."""
    for c in M.fixture()["cases"]:
        if c["count"] == 1000 and c["rounds"] == 90:
            got = committees.shuffled_indices(1000, M.generator_seeds()[c["seed"]], 90)
            assert M.list_digest(got) == c["sha256"], c["seed"]


@pytest.mark.parametrize("rounds", ROUNDS)
def test_small_windows(committees, lists, rounds):
    """Windows at both ends and a single position of a short list: through the table, whose rows
    are one ragged block short of four (the direct path takes lists of at least 65,536 blocks)."""
    want = lists[(1000, rounds)]
    for first, count in ((0, 3), (997, 3), (500, 1)):
        assert np.array_equal(committees.shuffled_indices(1000, SEED, rounds, first, count), want[first:first + count])


@pytest.mark.parametrize("rounds", ROUNDS)
def test_direct_path_index_count_near_2_to_32(committees, rounds):
    """Every counter byte the list can reach, and a pivot + n - index of 33 bits."""
    for first in (0, HUGE - 64):
        want = [M.get_shuffled_index(first + k, HUGE, SEED, rounds) for k in range(64)]
        assert committees.shuffled_indices(HUGE, SEED, rounds, first, 64).tolist() == want


@pytest.mark.parametrize("rounds", ROUNDS)
def test_windows_of_four_and_five(committees, lists, rounds):
    """ceil(1000 / 256) = 4: windows of 4 and of 5, where the two paths' hash counts cross, give
    the full list's slice."""
    want = lists[(1000, rounds)]
    for count in (4, 5):
        for first in (0, 254, 995):
            assert np.array_equal(committees.shuffled_indices(1000, SEED, rounds, first, count),
                                  want[first:first + count]), (first, count)
    assert len(committees.shuffled_indices(1000, SEED, rounds, 1000, 0)) == 0
    assert len(committees.shuffled_indices(0, SEED, rounds)) == 0


@pytest.mark.parametrize("rounds", ROUNDS)
def test_both_sides_of_the_path_rule(committees, dev, rounds):
    """The rule as measured: a window of at most ceil(n / 256) positions is hashed directly only in
    a list of at least 65,536 blocks.  n = 2^24 - 256 (65,535 blocks) goes through the table, one
    more index makes the 65,536th block and the same window direct; the workspace sizes show the
    path, the spec's loop checks the values."""
    L = dev.L
    for n, direct in ((2 ** 24 - 256, False), (2 ** 24 - 255, True)):
        blocks = (n + 255) // 256
        table_bytes = rounds * blocks * 32
        assert (L.bls381_shuffle_workspace_size(n, 5, rounds) < table_bytes) == direct
        assert L.bls381_shuffle_workspace_size(n, blocks + 1, rounds) >= table_bytes      # past the hash-count crossing
        for first in (0, n - 5):
            want = [M.get_shuffled_index(first + k, n, SEED, rounds) for k in range(5)]
            assert committees.shuffled_indices(n, SEED, rounds, first, 5).tolist() == want, (n, first)
    assert L.bls381_shuffle_workspace_size(HUGE, 64, rounds) < 4096                         # the 2^32 - 1 windows: direct
    assert L.bls381_shuffle_workspace_size(1000, 3, rounds) >= rounds * 4 * 32


def test_zero_rounds_is_the_identity(committees):
    assert committees.shuffled_indices(1000, SEED, 0).tolist() == list(range(1000))
    assert committees.shuffled_indices(1000, SEED, 0, 998, 2).tolist() == [998, 999]


def _active_set():
    rng = random.Random(0xB15_0300)
    return np.array(rng.sample(range(64), 50), dtype=np.uint32)     # 50 of 64 registry entries, scrambled


@pytest.mark.parametrize("rounds", ROUNDS)
def test_gather_compute_committee(committees, dev, rounds):
    import torch
    active = _active_set()
    assert sorted(active.tolist()) != active.tolist()
    d_active = dev.up(active)
    for committee_count in (1, 4, 7):
        bounds = committees.committee_bounds(50, committee_count)
        assert bounds[0] == 0 and bounds[-1] == 50 and len(bounds) == committee_count + 1
        for j in range(committee_count):
            want = M.compute_committee(active.tolist(), SEED, j, committee_count, rounds)
            assert committees.compute_committee(active, SEED, j, committee_count, rounds).tolist() == want
            first, count = int(bounds[j]), int(bounds[j + 1] - bounds[j])
            assert count == len(want)
            d_out = dev.empty(4 * count + 8)
            ws = dev.empty(dev.L.bls381_shuffle_workspace_size(50, count, rounds))
            assert dev.L.bls381_shuffle_device(50, SEED, rounds, first, count, d_active.data_ptr(), d_out.data_ptr(),
                                               ws.data_ptr(), dev.stream()) == 0
            torch.cuda.synchronize()
            got = dev.u32(d_out[:4 * count + 8])
            assert got[:count].tolist() == want and np.all(got[count:] == 0xEEEEEEEE)     # nothing past the window


def test_device_form_table_path_leaves_the_rest_alone(dev, lists):
    """A ragged window through the table path on device buffers: only out[0 .. count) is written."""
    import torch
    n, rounds, first, count = 1000, 90, 300, 333
    d_out = dev.empty(4 * count + 16)
    wsb = dev.L.bls381_shuffle_workspace_size(n, count, rounds)
    assert wsb >= 90 * 4 * 32 + 4 * 90
    ws = dev.empty(wsb)
    assert dev.L.bls381_shuffle_device(n, SEED, rounds, first, count, None, d_out.data_ptr(), ws.data_ptr(),
                                       dev.stream()) == 0
    torch.cuda.synchronize()
    got = dev.u32(d_out)
    assert np.array_equal(got[:count], lists[(n, rounds)][first:first + count]) and np.all(got[count:] == 0xEEEEEEEE)


def test_shuffle_bad_arguments(native, dev):
    L = dev.L
    out = np.zeros(8, dtype=np.uint32)
    ws = dev.empty(1 << 16)
    assert L.bls381_shuffle(2 ** 32, SEED, 90, 0, 1, None, cvp(out)) == native.EARG          # the 32-bit cap
    assert L.bls381_shuffle(10, SEED, 90, 8, 3, None, cvp(out)) == native.EARG               # first + count > n
    assert L.bls381_shuffle(10, SEED, 90, 11, 0, None, cvp(out)) == native.EARG
    assert L.bls381_shuffle(10, SEED, 90, 0, 2 ** 64 - 1, None, cvp(out)) == native.EARG
    assert L.bls381_shuffle(10, SEED, 256, 0, 1, None, cvp(out)) == native.EARG              # rounds > 255
    assert L.bls381_shuffle(10, None, 90, 0, 1, None, cvp(out)) == native.EARG               # NULL with sizes
    assert L.bls381_shuffle(10, SEED, 90, 0, 1, None, None) == native.EARG
    assert L.bls381_shuffle(0, None, 90, 0, 0, None, None) == 0                              # nothing to do
    assert L.bls381_shuffle(10, SEED, 255, 0, 8, None, cvp(out)) == 0
    assert out.tolist() == M.shuffled_list(10, SEED, 255)[:8].tolist()
    for bad in ((2 ** 32, SEED, 90, 0, 1), (10, SEED, 90, 8, 3), (10, SEED, 256, 0, 1), (10, None, 90, 0, 1)):
        assert L.bls381_shuffle_device(*bad, None, ws.data_ptr(), ws.data_ptr(), dev.stream()) == native.EARG
    assert L.bls381_shuffle_device(10, SEED, 90, 0, 1, None, None, ws.data_ptr(), dev.stream()) == native.EARG
    assert L.bls381_shuffle_device(10, SEED, 90, 0, 1, None, ws.data_ptr(), None, dev.stream()) == native.EARG
    assert L.bls381_shuffle_device(0, None, 90, 0, 0, None, None, None, dev.stream()) == 0
    assert L.bls381_shuffle_workspace_size(2 ** 32, 1, 90) == 0
    assert L.bls381_shuffle_workspace_size(10, 1, 256) == 0
    with pytest.raises(ValueError):
        from bls381_amd import committees
        committees.shuffled_indices(10, SEED, 90, 8, 3)


# --------------------------------------------------------------- attesting entries
class Atts:
    pass


@pytest.fixture(scope="module")
def atts():
    """40 attestations over committees of lengths 0, 1, 9, 128, 257 and 4,096 cut from one list of
    distinct entries; attestations 7 (a set padding bit) and 22 (a byte too many) have bad bitfields."""
    rng = random.Random(0xB15_0301)
    a = Atts()
    a.lens = [ATT_LENGTHS[k % 6] for k in range(40)]
    a.off = np.concatenate([[0], np.cumsum(a.lens)]).astype(np.uint32)
    total = int(a.off[-1])
    values = rng.sample(range(1 << 24), total - 1) + [0xFFFFFFFF]
    rng.shuffle(values)
    a.shuffled = np.array(values, dtype=np.uint32)
    a.committees = [a.shuffled[a.off[k]:a.off[k + 1]].tolist() for k in range(40)]
    a.agg = [M.random_bitfield(rng, n, rng.choice([0.2, 0.6, 1.0])) for n in a.lens]
    a.cust = [M.random_bitfield(rng, n, rng.choice([0.0, 0.3])) for n in a.lens]
    assert a.lens[7] == 1 and a.lens[22] == 257
    a.agg[7] = bytes([a.agg[7][0] | 0x02])
    a.agg[22], a.cust[22] = a.agg[22] + b"\x00", a.cust[22] + b"\x00"
    a.model = M.attesting_entries(a.committees, a.agg, a.cust)
    assert [k for k in range(40) if not a.model[1][k]] == [7, 22] and len(a.model[2]) > 8000
    return a


def test_attesting_entries_host_form(committees, atts):
    gko, ok, entries = committees.attesting_entries(atts.shuffled, atts.off[:-1], atts.lens, atts.agg, atts.cust)
    want_off, want_ok, want_entries = atts.model
    assert gko.tolist() == want_off and ok.tolist() == [bool(v) for v in want_ok]
    assert entries.dtype == np.uint32 and entries.tolist() == want_entries


def test_attesting_entries_device_form(native, dev, atts):
    import torch
    L = dev.L
    want_off, want_ok, want_entries = atts.model
    used = len(want_entries)
    boff = np.concatenate([[0], np.cumsum([len(b) for b in atts.agg])]).astype(np.uint32)
    coff, clen = atts.off[:-1].copy(), np.array(atts.lens, dtype=np.uint32)
    agg, cust = b"".join(atts.agg), b"".join(atts.cust)
    d_sh = dev.up(atts.shuffled)
    cap = used + 100
    d_ent = dev.empty(4 * cap)
    ws = dev.empty(L.bls381_attesting_entries_workspace_size(40, int(boff[-1])))
    gko, ok = np.full(81, 77, dtype=np.uint32), np.full(40, 77, dtype=np.uint8)
    args = lambda cap_: (40, cvp(coff), cvp(clen), cvp(boff), agg, cust, d_sh.data_ptr(), len(atts.shuffled), cvp(gko),
                         cvp(ok), d_ent.data_ptr(), cap_, ws.data_ptr(), dev.stream())
    assert L.bls381_attesting_entries_device(*args(cap)) == 0
    assert gko.tolist() == want_off and ok.tolist() == want_ok          # host outputs: complete on return
    torch.cuda.synchronize()
    raw = dev.u32(d_ent)
    assert raw[:used].tolist() == want_entries
    assert np.all(raw[used:] == 0xEEEEEEEE)                              # bytes past the used count are untouched
    assert L.bls381_attesting_entries_device(*args(used)) == 0           # an exact fit
    assert L.bls381_attesting_entries_device(*args(used - 1)) == native.EARG
    torch.cuda.synchronize()


def test_get_attesting_indices(committees):
    rng = random.Random(0xB15_0302)
    for n in (1, 9, 257):
        committee = rng.sample(range(1 << 20), n)
        bits = M.random_bitfield(rng, n, 0.5)
        assert committees.get_attesting_indices(committee, bits) == M.get_attesting_indices(committee, bits)
    assert committees.get_attesting_indices([], b"") == []
    with pytest.raises(AssertionError):
        committees.get_attesting_indices(list(range(9)), b"\xff\x02")    # a padding bit
    with pytest.raises(AssertionError):
        committees.get_attesting_indices(list(range(9)), b"\xff")        # too short
    with pytest.raises(ValueError):
        committees.get_attesting_indices(list(range(4097)), bytes(513))


def test_attesting_entries_bad_arguments(native, dev):
    L = dev.L
    sh = np.arange(5000, dtype=np.uint32)
    d_sh, d_ent, ws = dev.up(sh), dev.empty(4 * 5000), dev.empty(1 << 16)
    gko, ok = np.zeros(3, dtype=np.uint32), np.zeros(1, dtype=np.uint8)

    def call(coff, clen, boff, agg, cust, n_sh=5000, cap=5000, sh_ptr=d_sh.data_ptr(), ent=d_ent.data_ptr(),
             wsp=ws.data_ptr(), gko_=gko, ok_=ok):
        a = lambda v: np.array(v, dtype=np.uint32)
        c, l, b = a(coff), a(clen), a(boff)
        return L.bls381_attesting_entries_device(1, cvp(c), cvp(l), cvp(b), agg, cust, sh_ptr, n_sh,
                                                 None if gko_ is None else cvp(gko_), None if ok_ is None else cvp(ok_),
                                                 ent, cap, wsp, dev.stream())

    one = b"\xff" * 512
    assert call([0], [4096], [0, 512], one, bytes(512)) == 0 and gko.tolist() == [0, 4096, 4096]
    assert call([0], [4097], [0, 513], b"\xff" * 513, bytes(513)) == native.EARG         # over MAX_INDICES_PER_ATTESTATION
    assert call([905], [4096], [0, 512], one, bytes(512)) == native.EARG                 # slice outside n_shuffled
    assert call([0], [4096], [0, 512], one, bytes(512), n_sh=4095) == native.EARG
    assert call([0], [4096], [0, 512], one, bytes(512), cap=4095) == native.EARG         # cap below the popcount total
    assert call([0], [9], [2, 0], one, one) == native.EARG                                # descending bit offsets
    assert call([0], [9], [0, 2], None, b"\x00\x00") == native.EARG                       # NULL with nonzero sizes
    assert call([0], [9], [0, 2], b"\x01\x00", None) == native.EARG
    assert call([0], [9], [0, 2], b"\x01\x00", b"\x00\x00", sh_ptr=None) == native.EARG
    assert call([0], [9], [0, 2], b"\x01\x00", b"\x00\x00", ent=None) == native.EARG
    assert call([0], [9], [0, 2], b"\x01\x00", b"\x00\x00", wsp=None) == native.EARG
    assert call([0], [9], [0, 2], b"\x01\x00", b"\x00\x00", gko_=None) == native.EARG
    assert call([0], [9], [0, 2], b"\x01\x00", b"\x00\x00", ok_=None) == native.EARG
    assert call([0], [9], [0, 2], b"\x00\x00", b"\x00\x00", ent=None) == 0                # no members: nothing to write
    assert L.bls381_attesting_entries_device(0, None, None, None, None, None, None, 0, cvp(gko), None, None, 0, None,
                                             dev.stream()) == 0
    assert L.bls381_attesting_entries(0, None, None, None, None, None, None, 0, cvp(gko), None, None, 0) == 0
    assert L.bls381_attesting_entries(1, None, None, None, None, None, None, 0, cvp(gko), None, None, 0) == native.EARG
    import torch
    torch.cuda.synchronize()


# -------------------------------------------------------------------- end to end
def test_shuffle_to_verdicts_on_device_buffers(native, dev, committees):
    """64 registered keys, 50 active, four committees; shuffle -> attesting entries -> grouped
    registry verify on one stream, the member entries never on the host."""
    import torch
    from bls381_amd.registry import PubkeyRegistry
    import bls_oracle as O
    L = dev.L
    rng = random.Random(0xB15_0303)
    rounds, dom8 = 10, (2).to_bytes(8, "big")
    sks = [rng.randrange(1, O.r) for _ in range(64)]
    pks = native.privtopub_batch(b"".join(k.to_bytes(32, "big") for k in sks))
    active = _active_set()
    bounds = committees.committee_bounds(50, 4)
    model_committees = [M.compute_committee(active.tolist(), SEED, j, 4, rounds) for j in range(4)]
    # attestations: (committee, aggregation bits, custody bits, what happens after signing)
    plan = []
    for j in range(4):
        n = len(model_committees[j])
        agg = M.random_bitfield(rng, n, 0.6)
        plan.append([j, agg, bytes(len(agg)), None])
    n0 = len(model_committees[0])
    plan.append([0, bytes([0xFF] * ((n0 + 7) // 8 - 1) + [(1 << ((n0 - 1) % 8 + 1)) - 1]),
                 bytes([0b00100101]) + bytes((n0 + 7) // 8 - 1), None])          # members in both groups
    plan.append([1, plan[1][1], plan[1][2], "flip"])
    plan.append([2, plan[2][1], plan[2][2], "pad"])
    n_att = len(plan)
    msgs = [(rng.randbytes(32), rng.randbytes(32)) for _ in range(n_att)]
    sigs = []
    for a, (j, agg, cust, _) in enumerate(plan):
        g0, g1 = M.convert_to_indexed_sets(model_committees[j], agg, cust)
        assert g0 and (a != 4 or (len(g1) == 3 and len(g0) == n0 - 3))
        members = [(msgs[a][0], v) for v in g0] + [(msgs[a][1], v) for v in g1]
        parts = native.sign_batch(b"".join(m for m, _ in members),
                                  b"".join(sks[v].to_bytes(32, "big") for _, v in members), dom8 * len(members))
        sigs.append(native.aggregate_signatures(parts))
    for p in plan:                                                               # after signing
        if p[3] == "flip":
            p[1] = bytes([p[1][0] ^ 0x01]) + p[1][1:]
        elif p[3] == "pad":
            n = len(model_committees[p[0]])
            assert n % 8
            p[1] = p[1][:-1] + bytes([p[1][-1] | 0x80])
    expected = [True, True, True, True, True, False, False]
    want_off, want_ok, want_entries = M.attesting_entries([model_committees[p[0]] for p in plan], [p[1] for p in plan],
                                                          [p[2] for p in plan])
    assert want_ok == [1, 1, 1, 1, 1, 1, 0]
    # the oracle's own verdict on a good one, the one with both groups, and the flipped one
    for a in (0, 4, 5):
        groups = [want_entries[want_off[2 * a]:want_off[2 * a + 1]], want_entries[want_off[2 * a + 1]:want_off[2 * a + 2]]]
        aggs = [O.aggregate_pubkeys([pks[48 * v:48 * v + 48] for v in g]) for g in groups]
        assert O.verify_multiple(aggs, list(msgs[a]), sigs[a], 2) == expected[a]

    reg = PubkeyRegistry(64)
    try:
        assert list(reg.add([pks[48 * i:48 * i + 48] for i in range(64)])) == list(range(64))
        sp = dev.stream()
        d_active, d_sigs, d_doms = dev.up(active), dev.up(np.frombuffer(b"".join(sigs), dtype=np.uint8)), \
            dev.up(np.frombuffer(dom8 * n_att, dtype=np.uint8))
        d_shuffled, d_entries = dev.empty(4 * 50), dev.empty(4 * 50 * n_att)
        sws = dev.empty(L.bls381_shuffle_workspace_size(50, 50, rounds))
        coff = np.array([bounds[p[0]] for p in plan], dtype=np.uint32)
        clen = np.array([bounds[p[0] + 1] - bounds[p[0]] for p in plan], dtype=np.uint32)
        boff = np.concatenate([[0], np.cumsum([len(p[1]) for p in plan])]).astype(np.uint32)
        aws = dev.empty(L.bls381_attesting_entries_workspace_size(n_att, int(boff[-1])))
        gko, ok = np.zeros(2 * n_att + 1, dtype=np.uint32), np.zeros(n_att, dtype=np.uint8)
        call_off = np.arange(0, 2 * n_att + 1, 2, dtype=np.uint32)
        group_msgs = b"".join(m0 + m1 for m0, m1 in msgs)
        gws = dev.empty(L.bls381_verify_multiple_grouped_workspace_size(n_att, 2 * n_att, 50 * n_att, 32))
        d_v = dev.empty(n_att)
        native.check(L.bls381_shuffle_device(50, SEED, rounds, 0, 50, d_active.data_ptr(), d_shuffled.data_ptr(),
                                             sws.data_ptr(), sp))
        native.check(L.bls381_attesting_entries_device(
            n_att, cvp(coff), cvp(clen), cvp(boff), b"".join(p[1] for p in plan), b"".join(p[2] for p in plan),
            d_shuffled.data_ptr(), 50, cvp(gko), cvp(ok), d_entries.data_ptr(), 50 * n_att, aws.data_ptr(), sp))
        assert gko.tolist() == want_off and ok.tolist() == want_ok
        native.check(L.bls381_registry_verify_multiple_grouped_device(
            reg._h, n_att, cvp(call_off), 2 * n_att, cvp(gko), group_msgs, 32, d_entries.data_ptr(), d_sigs.data_ptr(),
            d_doms.data_ptr(), d_v.data_ptr(), gws.data_ptr(), sp))
        # the same call fed the model's entry lists from the host
        d_model = dev.up(np.array(want_entries + [0], dtype=np.uint32))
        d_v2 = dev.empty(n_att)
        moff = np.array(want_off, dtype=np.uint32)
        native.check(L.bls381_registry_verify_multiple_grouped_device(
            reg._h, n_att, cvp(call_off), 2 * n_att, cvp(moff), group_msgs, 32, d_model.data_ptr(), d_sigs.data_ptr(),
            d_doms.data_ptr(), d_v2.data_ptr(), gws.data_ptr(), sp))
        torch.cuda.synchronize()
        assert dev.u32(d_shuffled).tolist() == [v for c in model_committees for v in c]
        assert dev.u32(d_entries)[:len(want_entries)].tolist() == want_entries
        v, v2 = d_v.cpu().numpy().astype(bool).tolist(), d_v2.cpu().numpy().astype(bool).tolist()
        assert v == expected and v2 == expected
    finally:
        reg.close()
