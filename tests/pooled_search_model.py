"""Model of k_hash_cand_1's pooled try-and-increment search (bls381_kernels.hpp,
dev_hash_cand_1): the lane assignment and per-item resolution of one 64-lane wave.
tests/test_pooled_search_model.py proves it over random square patterns; tests/hash_search_cases.py
runs it over the square masks of tests/golden/hash_search.json to say what each composed wave does.
"""


def nth_set_bit(m, r):
    for b in range(64):
        if (m >> b) & 1:
            if r == 0:
                return b
            r -= 1
    raise AssertionError("rank out of range")


def pooled_search(is_square, valid, trace=None):
    """is_square(item, offset) -> bool; valid[lane]; returns (found offsets, rounds).
    trace: a list that receives each round's m, the number of unresolved items."""
    k = [0] * 64
    found = [-1 if valid[i] else 0 for i in range(64)]
    rounds = 0
    while True:
        P = sum(1 << i for i in range(64) if found[i] < 0)
        if P == 0:
            return found, rounds
        rounds += 1
        m = bin(P).count("1")
        if trace is not None:
            trace.append(m)
        t = [nth_set_bit(P, lane % m) for lane in range(64)]
        off = [k[t[lane]] + lane // m for lane in range(64)]
        B = sum(1 << lane for lane in range(64) if is_square(t[lane], off[lane]))
        for lane in range(64):
            if found[lane] < 0:
                r = bin(P & ((1 << lane) - 1)).count("1")
                first, cnt, j = -1, 0, r
                while j < 64:
                    if first < 0 and (B >> j) & 1:
                        first = cnt
                    j += m
                    cnt += 1
                if first >= 0:
                    found[lane] = k[lane] + first
                else:
                    k[lane] += cnt
