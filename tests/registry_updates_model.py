"""A Python restatement of process_registry_updates and initiate_validator_exit
(specs/core/0_beacon-chain.md:1480-1502, :1110-1128, :1081-1088, :1071-1075) over plain lists, in
the spec's own sequential form -- the scans and the sort are here, the closed forms are in the code
under test.  Pinned to tests/golden/registry_updates.json by tests/test_registry_updates_host.py.

Beyond the spec text: an exit_epoch or withdrawable_epoch that would pass 2^64 - 1 becomes
2^64 - 1 and its validator counts once in the status word (the engine's rule; the spec's integers
are unbounded).  The queue's own position is kept unbounded, apart from the stored epochs.
"""
FAR = 2 ** 64 - 1
NONE = 0xFFFFFFFF
MAINNET = {"MAX_EFFECTIVE_BALANCE": 32 * 10 ** 9, "EJECTION_BALANCE": 16 * 10 ** 9, "ACTIVATION_EXIT_DELAY": 4,
           "MIN_VALIDATOR_WITHDRAWABILITY_DELAY": 256, "MIN_PER_EPOCH_CHURN_LIMIT": 4, "CHURN_LIMIT_QUOTIENT": 65536}
CONSTANT_NAMES = ("MAX_EFFECTIVE_BALANCE", "EJECTION_BALANCE", "ACTIVATION_EXIT_DELAY",
                  "MIN_VALIDATOR_WITHDRAWABILITY_DELAY", "MIN_PER_EPOCH_CHURN_LIMIT", "CHURN_LIMIT_QUOTIENT")


def constants6(c):
    return [int(c[name]) for name in CONSTANT_NAMES]


def delayed(epoch, c):
    return epoch + 1 + c["ACTIVATION_EXIT_DELAY"]


def is_active(act, ext, epoch):
    return act <= epoch < ext


def churn_limit(act, ext, cur, c):
    active = sum(1 for a, x in zip(act, ext) if is_active(a, x, cur))
    return max(c["MIN_PER_EPOCH_CHURN_LIMIT"], active // c["CHURN_LIMIT_QUOTIENT"]), active


def exit_queue(act, ext, cur, c):
    """(exit_queue_epoch, exit_queue_churn, churn limit, active count) as :1119-1123 see them."""
    limit, active = churn_limit(act, ext, cur, c)
    epochs = [x for x in ext if x != FAR]
    e0 = max(epochs + [delayed(cur, c)])
    return e0, sum(1 for x in ext if x == e0), limit, active


def registry_updates(elig, act, ext, wd, eff, cur, fin, c):
    """Returns (indices, values, summary) as bls381_registry_updates does; None for arguments it
    rejects."""
    n = len(eff)
    if c["CHURN_LIMIT_QUOTIENT"] == 0 or delayed(cur, c) > FAR or delayed(fin, c) > FAR:
        return None
    limit, active = churn_limit(act, ext, cur, c)
    if limit == 0:
        return None
    new_elig, new_act, new_ext, new_wd = list(elig), list(act), list(ext), list(wd)
    e0 = exit_queue(act, ext, cur, c)[0]
    # the largest exit epoch and how many hold it, kept as the scans of :1120-1122 would find them
    # (unbounded integers: an epoch past 2^64 - 1 is still an epoch to the queue)
    exited = [x for x in ext if x != FAR]
    peak = max(exited) if exited else None
    held = sum(1 for x in exited if x == peak)
    ejected = status = 0
    for i in range(n):
        if new_elig[i] == FAR and eff[i] >= c["MAX_EFFECTIVE_BALANCE"]:
            new_elig[i] = cur
        if is_active(act[i], ext[i], cur) and eff[i] <= c["EJECTION_BALANCE"] and ext[i] == FAR:
            # initiate_validator_exit
            q = delayed(cur, c) if peak is None else max(peak, delayed(cur, c))
            if (held if q == peak else 0) >= limit:
                q += 1
            peak, held = (q, held + 1) if q == peak else (q, 1)
            w = q + c["MIN_VALIDATOR_WITHDRAWABILITY_DELAY"]
            new_ext[i], new_wd[i] = min(q, FAR), min(w, FAR)
            status += q > FAR or w > FAR
            ejected += 1
    queue = sorted([i for i in range(n) if new_elig[i] != FAR and act[i] >= delayed(fin, c)], key=lambda i: new_elig[i])
    for i in queue[:limit]:
        if new_act[i] == FAR:
            new_act[i] = delayed(cur, c)
    values = [[new_elig[i], new_act[i], new_ext[i], new_wd[i]] for i in range(n)]
    old = [[elig[i], act[i], ext[i], wd[i]] for i in range(n)]
    indices = [i if values[i] != old[i] else NONE for i in range(n)]
    summary = [sum(1 for i in range(n) if new_elig[i] != elig[i]), ejected, sum(1 for i in range(n) if new_act[i] != act[i]),
               sum(1 for x in indices if x != NONE), active, limit, e0, status]
    return indices, values, summary
