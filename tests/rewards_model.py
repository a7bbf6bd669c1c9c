"""The epoch rewards restated in Python integers: what csrc/bls381_rewards.hpp computes, device
winner rule and overflow rules included (include/bls381.h "epoch rewards").  Checked against
tests/golden/epoch_rewards.json (the reference's spec text, make_epoch_rewards_vectors.py) by
test_rewards_host.py; the native code is checked against this model, never the other way round.
"""
import hashlib
import json
import os
import struct

U64 = 1 << 64
NONE = 0xFFFFFFFF
SOURCE, TARGET, HEAD, WINNER, MEMBER = 1, 2, 4, 8, 16
DEFAULT_CROSSLINK = (0, 0, 0, bytes(32), bytes(32))
CONSTANT_NAMES = ("BASE_REWARD_FACTOR", "BASE_REWARDS_PER_EPOCH", "PROPOSER_REWARD_QUOTIENT",
                  "MIN_ATTESTATION_INCLUSION_DELAY", "MIN_EPOCHS_TO_INACTIVITY_PENALTY", "INACTIVITY_PENALTY_QUOTIENT")
_FIXTURE = None


def fixture():
    global _FIXTURE
    if _FIXTURE is None:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "epoch_rewards.json")) as f:
            _FIXTURE = json.load(f)
    return _FIXTURE


def digest(values):
    return hashlib.sha256(struct.pack("<%dQ" % len(values), *values)).hexdigest()


def matches(stored, values):
    """A stored list, or its digest (the 301-validator states)."""
    return stored["sha256"] == digest(values) if isinstance(stored, dict) else stored == list(values)


# ---- arithmetic: the native saturation rules ------------------------------------------------
class Count:
    def __init__(self):
        self.n = 0


def mul_div(a, b, d, ovf):
    q = a * b // d
    if q >= U64:
        ovf.n += 1
        return U64 - 1
    return q


def sat_add(a, b, ovf):
    if a + b >= U64:
        ovf.n += 1
        return U64 - 1
    return a + b


def isqrt(n):
    x, y = n, (n + 1) // 2
    while y < x:
        x, y = y, (y + n // y) // 2
    return x


# ---- the host work the device rules assume ----------------------------------------------------
def assign_candidates(atts):
    """One committee's attestations in list order, each a dict with `crosslink` (shard, start_epoch,
    end_epoch, parent_root, data_root) and `passes_filter`.  Returns (candidate id per attestation,
    candidate count, the crosslink of each id) such that "largest balance, then largest id" is
    the spec's max(key=(balance, data_root)) with the first in list order winning among equal keys:
    ids ascend by data_root and, among equal data_roots, by descending first appearance.  Without a
    crosslink that passes the filter the attestations equal to Crosslink() form candidate 0."""
    passing = []
    for a in atts:
        if a["passes_filter"] and a["crosslink"] not in passing:
            passing.append(a["crosslink"])
    if passing:
        order = sorted(range(len(passing)), key=lambda k: (passing[k][4], -k))
        ids = {passing[k]: rank for rank, k in enumerate(order)}
        return [ids.get(a["crosslink"], NONE) for a in atts], len(passing), [passing[k] for k in order]
    cand = [0 if a["crosslink"] == DEFAULT_CROSSLINK else NONE for a in atts]
    return cand, (1 if 0 in cand else 0), [DEFAULT_CROSSLINK] if 0 in cand else []


def bit(bits, j):
    return (bits[j // 8] >> (j % 8)) & 1


# ---- call 1: votes ----------------------------------------------------------------------------
def votes(n, committees, atts, cand_count, slashed, eff):
    """committees[c]: the member indices; atts[c]: the committee's attestations in list order, dicts
    with bits (bytes), flags (bit 0 target, bit 1 head), delay, proposer, cand."""
    out = {"votes": [0] * n, "incl_delay": [0] * n, "incl_proposer": [0] * n, "committee_of": [NONE] * n,
           "winner": [], "winner_balance": [], "committee_balance": [], "totals": [0, 0, 0]}
    for c, members in enumerate(committees):
        balance = 0
        for j, v in enumerate(members):
            if v >= n:
                continue
            balance += eff[v]
            vt = MEMBER
            mine = [a for a in atts[c] if bit(a["bits"], j)]
            if not slashed[v]:
                if mine:
                    vt |= SOURCE
                if any(a["flags"] & 1 for a in mine):
                    vt |= TARGET
                if any(a["flags"] & 2 for a in mine):
                    vt |= HEAD
            out["votes"][v] = vt
            out["committee_of"][v] = c
            for g in range(3):
                if vt & (1 << g):
                    out["totals"][g] += eff[v]
            if vt & SOURCE:
                first = min(mine, key=lambda a: a["delay"])   # the first among equal delays
                out["incl_delay"][v], out["incl_proposer"][v] = first["delay"], first["proposer"]
        best, best_balance, best_set = NONE, 0, []
        for k in range(cand_count[c]):
            union = [v for j, v in enumerate(members)
                     if v < n and not slashed[v] and any(a["cand"] == k and bit(a["bits"], j) for a in atts[c])]
            b = sum(eff[v] for v in union)
            if best == NONE or b >= best_balance:
                best, best_balance, best_set = k, b, union
        for v in best_set:
            out["votes"][v] |= WINNER
        out["winner"].append(best)
        out["winner_balance"].append(best_balance)
        out["committee_balance"].append(balance)
    for g in range(3):
        out["totals"][g] %= U64
    return out


# ---- call 2: deltas ---------------------------------------------------------------------------
def deltas(K, which, previous_epoch, finalized_epoch, total_balance, act, ext, wd, slashed, eff, balances, vo,
           n_committees=None):
    """K: the six constants in CONSTANT_NAMES order; vo: the outputs of votes().  Returns rewards,
    penalties, new_balances, overflows."""
    brf, brpe, prq, mid, meip, ipq = K
    n = len(eff)
    nc = len(vo["winner_balance"]) if n_committees is None else n_committees
    total = max(1, total_balance)
    root = isqrt(total)
    ovf = Count()
    rewards, penalties, prop = [0] * n, [0] * n, [0] * n
    for i in range(n):
        vt = vo["votes"][i]
        base = mul_div(eff[i], brf, root, ovf) // brpe
        r = p = 0
        if which & 1:
            eligible = act[i] <= previous_epoch < ext[i] or (slashed[i] and previous_epoch + 1 < wd[i])
            if eligible:
                for g in range(3):
                    if vt & (1 << g):
                        r = sat_add(r, mul_div(base, max(1, vo["totals"][g]), total, ovf), ovf)
                    else:
                        p = sat_add(p, base, ovf)
            if vt & SOURCE:
                addend, proposer = base // prq, vo["incl_proposer"][i]
                if proposer >= n or addend >= 1 << 32:
                    ovf.n += 1
                else:
                    prop[proposer] += addend
                if vo["incl_delay"][i] == 0:
                    ovf.n += 1
                else:
                    r = sat_add(r, mul_div(base, mid, vo["incl_delay"][i], ovf), ovf)
            delay = previous_epoch - finalized_epoch
            if eligible and delay > meip:
                p = sat_add(p, mul_div(brpe, base, 1, ovf), ovf)
                if not vt & TARGET:
                    p = sat_add(p, mul_div(eff[i], delay, ipq, ovf), ovf)
        if which & 2:
            c = vo["committee_of"][i]
            if c != NONE:
                if c >= nc:
                    ovf.n += 1
                elif vt & WINNER:
                    r = sat_add(r, mul_div(base, max(1, vo["winner_balance"][c]), max(1, vo["committee_balance"][c]), ovf), ovf)
                else:
                    p = sat_add(p, base, ovf)
        rewards[i], penalties[i] = r, p
    new = []
    for i in range(n):
        rewards[i] = sat_add(rewards[i], prop[i], ovf)
        up = sat_add(balances[i], rewards[i], ovf)
        new.append(up - penalties[i] if up > penalties[i] else 0)
    return rewards, penalties, new, ovf.n


# ---- call 3: slashings ------------------------------------------------------------------------
def slashings(slashed, wd, eff, balances, current_epoch, total_penalties, total_balance, exit_length, quotient):
    total = max(1, total_balance)
    out = []
    for i, b in enumerate(balances):
        if slashed[i] and current_epoch == wd[i] - exit_length // 2:
            penalty = max(eff[i] * min(total_penalties * 3, total) // total, eff[i] // quotient)
            b = 0 if penalty > b else b - penalty
        out.append(b)
    return out


# ---- call 4: the hysteresis -------------------------------------------------------------------
def hysteresis(balances, eff, increment, max_effective_balance):
    """indices, values, changed."""
    indices, values = [], []
    for i, (b, e) in enumerate(zip(balances, eff)):
        v = e
        if b < e or e + 3 * (increment // 2) < b:
            v = min(b - b % increment, max_effective_balance)
        indices.append(i if v != e else NONE)
        values.append(v)
    return indices, values, sum(1 for x in indices if x != NONE)


# ---- fixture cases as the calls' inputs ---------------------------------------------------------
def case_constants(fx, case):
    k = fx["supplied"]["constants"][case["preset"]]
    return k, [k[name] for name in CONSTANT_NAMES]


def case_attestations(case):
    """Per committee (in `shards` order) the attestations in list order, with candidate ids."""
    per = [[] for _ in case["shards"]]
    for a in case["attestations"]:
        x = a["crosslink"]
        per[case["shards"].index(a["shard"])].append({
            "bits": bytes.fromhex(a["bits"]), "flags": int(a["target"]) | int(a["head"]) << 1, "delay": a["inclusion_delay"],
            "proposer": a["proposer_index"], "passes_filter": a["passes_filter"],
            "crosslink": (x[0], x[1], x[2], bytes.fromhex(x[3]), bytes.fromhex(x[4]))})
    cand_count, crosslinks = [], []
    for atts in per:
        cand, k, links = assign_candidates(atts)
        for a, c in zip(atts, cand):
            a["cand"] = c
        cand_count.append(k)
        crosslinks.append(links)
    return per, cand_count, crosslinks


def case_votes(case):
    per, cand_count, crosslinks = case_attestations(case)
    vo = votes(case["n"], case["committees"], per, cand_count, case["slashed"], case["effective_balances"])
    return vo, per, cand_count, crosslinks


def case_deltas(fx, case, vo, which, balances=None):
    _, K = case_constants(fx, case)
    return deltas(K, which, case["previous_epoch"], case["finalized_epoch"], case["total_active_balance"],
                  case["activation_epochs"], case["exit_epochs"], case["withdrawable_epochs"], case["slashed"],
                  case["effective_balances"], case["balances"] if balances is None else balances, vo)
