"""Inputs for the epoch-rewards tests (test_rewards_host.py, test_rewards_gpu.py): synthetic
committees and attestations at the byte, word, wave and workgroup edges, totals above 2^57, one
case per overflow kind, and the packing of model inputs into the arrays the native calls take.
Expected results always come from rewards_model.py."""
import random

import numpy as np

import rewards_model as M

ETH = 10 ** 9
U64 = 1 << 64
FAR = U64 - 1
MAINNET_K = [32, 5, 8, 4, 4, 1 << 25]     # CONSTANT_NAMES order, configs/constant_presets/mainnet.yaml
COMMITTEE_LENGTHS = [1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 4096]
BIT_PATTERNS = ("none", "all", "alternating", "last")
RECORD = 121                                 # serialized Validator: the fields' offsets below
OFF_ACTIVATION, OFF_EXIT, OFF_WITHDRAWABLE, OFF_SLASHED, OFF_EFFECTIVE = 88, 96, 104, 112, 113


def pattern_bits(pattern, m, rng=None):
    if pattern == "none":
        return [0] * m
    if pattern == "all":
        return [1] * m
    if pattern == "alternating":
        return [j & 1 for j in range(m)]
    if pattern == "last":
        return [int(j == m - 1) for j in range(m)]
    return [int(rng.random() < 0.5) for _ in range(m)]


def bitfield(bits):
    out = bytearray((len(bits) + 7) // 8)
    for j, b in enumerate(bits):
        if b:
            out[j // 8] |= 1 << (j % 8)
    return bytes(out)


def synth_votes(seed, lens, n, n_atts, n_cands, patterns=("random",), big=False, gap=0):
    """Committees of the given lengths over a random subset of n validators (the rest sit in no
    committee), n_atts[c] attestations and n_cands[c] candidates each; attestation a of a committee
    takes patterns[a % len].  big: effective balances near 2^57 / members, so that sums pass 2^57.
    gap: unused entries of the shuffled list between committees.  Returns a dict of model inputs."""
    rng = random.Random(seed)
    total = sum(lens)
    assert total <= n
    perm = rng.sample(range(n), total)
    committees, at = [], 0
    for m in lens:
        committees.append(perm[at:at + m])
        at += m
    slashed = [int(rng.random() < 0.2) for _ in range(n)]
    if big:
        eff = [rng.randrange(1 << 56, 1 << 58) // max(1, total // 4) for _ in range(n)]
    else:
        eff = [rng.choice([0, 1, 16, 31, 32, 32]) * ETH for _ in range(n)]
    atts = []
    for c, m in enumerate(lens):
        mine = []
        for a in range(n_atts[c]):
            bits = pattern_bits(patterns[a % len(patterns)], m, rng)
            mine.append({"bits": bitfield(bits), "flags": rng.randrange(4), "delay": rng.choice([1, 1, 2, 3, 3, 7]),
                         "proposer": rng.randrange(n),
                         "cand": rng.choice(list(range(n_cands[c])) + [M.NONE]) if n_cands[c] else M.NONE})
        atts.append(mine)
    return {"n": n, "committees": committees, "atts": atts, "cand_count": list(n_cands), "slashed": slashed, "eff": eff,
            "gap": gap}


def pack_votes(v):
    """The arrays of bls381_epoch_votes for a dict of synth_votes / the fixture."""
    gap = v.get("gap", 0)
    coff, clen, shuffled = [], [], []
    for members in v["committees"]:
        shuffled += [0xFFFFFFF0] * gap           # never read: outside every slice
        coff.append(len(shuffled))
        clen.append(len(members))
        shuffled += members
    att_off, bits_off, bits, flags, delay, proposer, cand = [0], [0], b"", [], [], [], []
    for mine in v["atts"]:
        for a in mine:
            bits += a["bits"]
            bits_off.append(len(bits))
            flags.append(a["flags"])
            delay.append(a["delay"])
            proposer.append(a["proposer"])
            cand.append(a["cand"])
        att_off.append(len(flags))
    u32 = lambda x: np.array(x, dtype=np.uint32)   # noqa: E731
    return {"coff": u32(coff), "clen": u32(clen), "shuffled": u32(shuffled), "att_off": u32(att_off),
            "bits_off": u32(bits_off), "bits": np.frombuffer(bits + b"\0", dtype=np.uint8).copy(),
            "flags": np.array(flags + [0], dtype=np.uint8), "delay": np.array(delay + [0], dtype=np.uint64),
            "proposer": u32(proposer + [0]), "cand": u32(cand + [0]), "cand_count": u32(v["cand_count"] + [0]),
            "slashed": np.array(v["slashed"] + [0], dtype=np.uint8), "eff": np.array(v["eff"] + [0], dtype=np.uint64)}


def records(act, ext, wd, slashed, eff, seed=0):
    """Serialized Validator records (121 bytes) with the five fields set and random bytes elsewhere."""
    rng = np.random.default_rng(seed)
    n = len(eff)
    buf = rng.integers(0, 256, size=(n, RECORD), dtype=np.uint8)
    for off, col in ((OFF_ACTIVATION, act), (OFF_EXIT, ext), (OFF_WITHDRAWABLE, wd), (OFF_EFFECTIVE, eff)):
        buf[:, off:off + 8] = np.array(col, dtype=np.uint64).astype("<u8").view(np.uint8).reshape(n, 8)
    buf[:, OFF_SLASHED] = np.array(slashed, dtype=np.uint8)
    return np.ascontiguousarray(buf.reshape(-1))


def synth_registry(seed, n, previous_epoch, eff=None, slashed=None):
    """activation / exit / withdrawable epochs around previous_epoch, and balances."""
    rng = random.Random(seed)
    act = [rng.choice([0, 0, 0, previous_epoch, previous_epoch + 1, FAR]) for _ in range(n)]
    ext = [rng.choice([FAR, FAR, FAR, previous_epoch, previous_epoch + 1, previous_epoch + 3]) for _ in range(n)]
    wd = [rng.choice([FAR, previous_epoch + 1, previous_epoch + 2, previous_epoch + 33, 0]) for _ in range(n)]
    eff = eff if eff is not None else [rng.choice([0, 1, 16, 31, 32, 32]) * ETH for _ in range(n)]
    slashed = slashed if slashed is not None else [int(rng.random() < 0.2) for _ in range(n)]
    bal = [rng.choice([e, e + 1, e + 2 * ETH, max(e, 5) - 5, 0, 1, 99999]) for e in eff]
    return act, ext, wd, slashed, eff, bal


def overflow_cases():
    """One case per overflow kind: name -> keyword arguments of rewards_model.deltas (vo included).
    Two validators; validator 0 attests, is active and has the winning crosslink."""
    def base():
        vo = {"votes": [31, 16], "incl_delay": [1, 0], "incl_proposer": [1, 0], "committee_of": [0, 0],
              "winner_balance": [32 * ETH], "committee_balance": [64 * ETH], "totals": [32 * ETH] * 3}
        return {"K": list(MAINNET_K), "which": 3, "previous_epoch": 8, "finalized_epoch": 7,
                "total_balance": 64 * ETH, "act": [0, 0], "ext": [FAR, FAR], "wd": [FAR, FAR], "slashed": [0, 0],
                "eff": [32 * ETH, 32 * ETH], "balances": [32 * ETH, 32 * ETH], "vo": vo}
    cases = {}
    c = base()                                   # base reward: eff * factor / sqrt(total) >= 2^64
    c["eff"][0], c["K"][0], c["total_balance"] = U64 - 1, U64 - 1, 1
    cases["quotient"] = c
    c = base()                                   # three source/target/head rewards of nearly 2^64 each
    c["eff"][0], c["K"][0], c["K"][1], c["total_balance"] = U64 - 1, 1, 1, 1
    c["vo"]["totals"] = [1, 1, 1]
    cases["sum"] = c
    c = base()                                   # increase_balance wraps
    c["balances"][0] = U64 - 5
    cases["increase"] = c
    c = base()                                   # a proposer addend of 2^32 or more
    c["eff"][0], c["total_balance"], c["K"][2] = 1 << 40, 1, 1
    cases["addend"] = c
    c = base()                                   # untrusted indices and delays
    c["vo"]["incl_proposer"][0] = 2
    cases["proposer_index"] = c
    c = base()
    c["vo"]["incl_delay"][0] = 0
    cases["zero_delay"] = c
    c = base()
    c["vo"]["committee_of"][1] = 1
    cases["committee_index"] = c
    return cases


def slashing_edges():
    """Withdrawable epochs around the condition, penalties on both sides of total / 3 and of the
    minimum, values near 2^64."""
    cur, half = 9, 32
    rows = []
    for wd in (cur + half, cur + half - 1, cur + half + 1, 0, half - 1, U64 - 1):
        for sl in (0, 1):
            for eff in (0, 32 * ETH, U64 - 1):
                for bal in (0, 10 ** 9, U64 - 1):
                    rows.append((sl, wd, eff, bal))
    return cur, 2 * half, rows


def hysteresis_edges():
    inc, top = 10 ** 9, 32 * 10 ** 9
    rows = []
    for e in (0, inc, 31 * inc, top):
        for d in (0, 1, -1, inc // 2, 3 * (inc // 2) - 1, 3 * (inc // 2), 3 * (inc // 2) + 1, 2 * inc, -inc, 5 * inc):
            rows.append((max(0, e + d), e))
    rows += [(U64 - 1, U64 - 1), (U64 - 1, U64 - 2), (U64 - 1, U64 - 1 - 3 * (inc // 2)), (U64 - 1, U64 - 2 - 3 * (inc // 2)), (0, U64 - 1)]
    return inc, top, rows
