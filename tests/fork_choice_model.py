"""The fork choice in plain Python: the restatement the engine is tested against
(csrc/bls381_forkchoice.hpp), pinned to the reference's spec text by
tests/golden/fork_choice.json (test_fork_choice_host.py).

* the key rule: a message is (slot << 32) | (0xFFFFFFFF - seq) with a target node, seq numbering the
  attestations over the life of the store in the order they were handed in; the larger key wins
* the vote counts: direct weights per node, laid out in preorder, one prefix sum, a node's count
  the difference over its subtree's range
* the descent: from the start node, the child with the largest (count, root) until there is none

A call the engine rejects returns None and changes nothing.
"""
NONE = 0xFFFFFFFF
MAX64 = 2 ** 64 - 1
SLOT_LIMIT = 2 ** 32
SEQ_LIMIT = 2 ** 32 - 1
BLOCK_LIMIT = 1 << 24


class Store:
    def __init__(self, validator_capacity, block_capacity):
        assert 0 < validator_capacity < 2 ** 32 and 0 < block_capacity <= BLOCK_LIMIT
        self.vcap, self.bcap, self.seq = validator_capacity, block_capacity, 0
        self.root, self.parent, self.slot, self.ids = [], [], [], {}
        self.key = [0] * validator_capacity
        self.target = [NONE] * validator_capacity

    # ---- blocks ------------------------------------------------------------------------------------
    def add_blocks(self, roots, parent_roots, slots):
        """The node ids, or None (and no block of the call is added)."""
        before = len(self.root)
        out = []
        for r, pr, s in zip(roots, parent_roots, slots):
            r = bytes(r)
            if r in self.ids:
                out.append(self.ids[r])
                continue
            p = NONE
            ok = True
            if self.root:
                p = self.ids.get(bytes(pr), NONE)
                ok = p != NONE and s > self.slot[p]
            if not ok or s >= SLOT_LIMIT or len(self.root) >= self.bcap:
                for gone in self.root[before:]:
                    del self.ids[gone]
                del self.root[before:], self.parent[before:], self.slot[before:]
                return None
            self.ids[r] = len(self.root)
            out.append(len(self.root))
            self.root.append(r), self.parent.append(p), self.slot.append(s)
        return out

    def node(self, root):
        return self.ids.get(bytes(root), NONE)

    # ---- latest messages ---------------------------------------------------------------------------
    def on_attestations(self, att_off, entries, slots, targets, ok=None):
        """How many members were skipped (at or above the capacity), or None."""
        n_att = len(slots)
        if self.seq + n_att > SEQ_LIMIT:
            return None
        for a in range(n_att):
            if att_off[a + 1] < att_off[a] or slots[a] >= SLOT_LIMIT or targets[a] >= len(self.root):
                return None
        skipped = 0
        for a in range(n_att):
            key = (slots[a] << 32) | (0xFFFFFFFF - (self.seq + a))
            if ok is not None and not ok[a]:
                continue
            for v in entries[att_off[a]:att_off[a + 1]]:
                if v >= self.vcap:
                    skipped += 1
                elif key > self.key[v]:
                    self.key[v], self.target[v] = key, targets[a]
        self.seq += n_att
        return skipped

    def latest(self, first, n):
        if first > self.vcap or n > self.vcap - first:
            return None
        return [k >> 32 for k in self.key[first:first + n]], self.target[first:first + n]

    def prune(self, anchor):
        if anchor >= len(self.root):
            return None
        new = {}
        for i in range(anchor, len(self.root)):
            if i == anchor or self.parent[i] in new:
                new[i] = len(new)
        kept = sorted(new)
        self.parent = [NONE if i == anchor else new[self.parent[i]] for i in kept]
        self.root, self.slot = [self.root[i] for i in kept], [self.slot[i] for i in kept]
        self.ids = {r: i for i, r in enumerate(self.root)}
        self.target = [new.get(t, NONE) for t in self.target]
        return True

    # ---- the head ----------------------------------------------------------------------------------
    def preorder(self):
        """(pre, size): the preorder position of every node, children in id order, and its subtree's size."""
        B = len(self.root)
        size = [1] * B
        for i in range(B - 1, 0, -1):
            size[self.parent[i]] += size[i]
        pre, nxt = [0] * B, [1] * B
        for i in range(1, B):
            p = self.parent[i]
            pre[i] = nxt[p]
            nxt[p] += size[i]
            nxt[i] = pre[i] + 1
        return pre, size

    def vote_counts(self, activation, exit_, effective, epoch):
        """(counts saturated at 2^64 - 1, how many were)."""
        B = len(self.root)
        direct = [0] * B
        for i in range(len(effective)):
            t = self.target[i]
            if t != NONE and activation[i] <= epoch < exit_[i]:
                direct[t] += effective[i]
        pre, size = self.preorder()
        prefix = [0] * (B + 1)
        for b in range(B):
            prefix[pre[b] + 1] = direct[b]
        for p in range(B):
            prefix[p + 1] += prefix[p]
        counts = [prefix[pre[b] + size[b]] - prefix[pre[b]] for b in range(B)]
        return [min(c, MAX64) for c in counts], sum(c > MAX64 for c in counts)

    def head(self, start, activation, exit_, effective, epoch):
        """(head node, counts, status), or None."""
        if start >= len(self.root) or len(effective) > self.vcap:
            return None
        counts, status = self.vote_counts([int(x) for x in activation], [int(x) for x in exit_],
                                          [int(x) for x in effective], int(epoch))
        children = [[] for _ in self.root]
        for i in range(1, len(self.root)):
            children[self.parent[i]].append(i)
        head = start
        while children[head]:
            head = max(children[head], key=lambda b: (counts[b], self.root[b]))
        return head, counts, status


def lmd_ghost(blocks, log, start, activation, exit_, effective, epoch):
    """One-shot: blocks as (root, parent index, slot), log as (slot, target, members)."""
    s = Store(max(1, len(effective)), max(1, len(blocks)))
    assert s.add_blocks([b[0] for b in blocks], [blocks[b[1]][0] if b[1] != NONE else bytes(32) for b in blocks],
                        [b[2] for b in blocks]) is not None
    off, entries = [0], []
    for _, _, members in log:
        entries += list(members)
        off.append(len(entries))
    assert s.on_attestations(off, entries, [a[0] for a in log], [a[1] for a in log]) is not None
    return s, s.head(start, activation, exit_, effective, epoch)
