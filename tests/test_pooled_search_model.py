"""Model of k_hash_cand_1's pooled try-and-increment search (bls381_kernels.hpp,
dev_hash_cand_1; the model: tests/pooled_search_model.py): the lane assignment and per-item
resolution, simulated for a 64-lane wave over random square patterns.  Each item must end with its lowest square offset -- the
spec's candidate order (bls_signature.md:74-86) -- whatever the other items do, and the
wave must finish in far fewer rounds than a lane-per-item loop's slowest item.
"""
import random

from pooled_search_model import pooled_search


def test_pooled_search_finds_first_square():
    rng = random.Random(0x5EA2C4)
    total_rounds = 0
    for trial in range(300):
        squares = [[rng.random() < 0.5 for _ in range(200)] for _ in range(64)]
        if trial % 7 == 0:                       # some items with long runs of non-squares
            for i in rng.sample(range(64), 5):
                run = rng.randrange(10, 60)
                squares[i][:run] = [False] * run
        valid = [True] * 64 if trial % 5 else [i < rng.randrange(1, 64) for i in range(64)]
        found, rounds = pooled_search(lambda i, o: squares[i][o], valid)
        total_rounds += rounds
        for i in range(64):
            if valid[i]:
                assert found[i] == squares[i].index(True), (trial, i)
    # a lane-per-item loop needs ~7.3 rounds per wave at probability 1/2; the pool needs ~3
    assert total_rounds / 300 < 4.5
