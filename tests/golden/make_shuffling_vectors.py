"""Pin the shuffle to the reference's own spec text: tests/golden/shuffling.json.

The reference ships a generator for shuffling vectors (test_generators/shuffling/main.py) but
not its output, and the generator needs the built pyspec package.  This script takes the same
functions mechanically from the spec's text instead: the ```python blocks of
specs/core/0_beacon-chain.md that define `get_shuffled_index`, `compute_committee`,
`int_to_bytes` and `bytes_to_int`, pulled by the fence rule of the reference's extractor
(scripts/function_puller.py:40-44: a line starting '```python' opens a block, '```' closes it;
see make_spec_text_vectors.py) and run unmodified.  What the text leaves to its surroundings is
supplied here and named in the output:
  * hash = SHA-256 (0_beacon-chain.md:591-595)
  * SHUFFLE_ROUND_COUNT from configs/constant_presets/{minimal,mainnet}.yaml
  * the annotation names ValidatorIndex = int, Bytes32 = bytes, List = typing.List

Cases: the generator's own (main.py:18-20) -- seeds hash(int_to_bytes(k, 4)) for k in 0..29,
counts [0, 1, 2, 3, 5, 10, 33, 100, 1000] -- under both round counts, 540 in all.  Each case
records the SHA-256 of its list packed as little-endian u32; the list itself is stored for seeds
0..3 at counts <= 100 and for seed 0 at count 1000.  Two compute_committee splits of seed 0's
1000 (over a non-identity index list) are recorded too.  Only outputs are stored, none of the
spec's text.

Run (in the build container, where the reference checkout exists):
    python tests/golden/make_shuffling_vectors.py
"""
import hashlib
import json
import os
import re
import struct
import typing

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("BLS381_REFERENCE", "/root/reference")
SPEC = os.path.join(REF, "specs", "core", "0_beacon-chain.md")
WANTED = ("get_shuffled_index", "compute_committee", "int_to_bytes", "bytes_to_int")
COUNTS = [0, 1, 2, 3, 5, 10, 33, 100, 1000]     # test_generators/shuffling/main.py:19
N_SEEDS = 30                                     # main.py:18


def pull_blocks():
    """The spec's python blocks that define the wanted functions, by the extractor's fence rule."""
    blocks, cur = [], None
    for line in open(SPEC).readlines():
        line = line.rstrip()
        if line[:9] == "```python":
            cur = []
        elif line[:3] == "```":
            if cur is not None:
                blocks.append("\n".join(cur))
            cur = None
        elif cur is not None:
            cur.append(line)
    picked = {}
    for b in blocks:
        m = re.match(r"def (\w+)\(", b)
        if m and m.group(1) in WANTED:
            assert m.group(1) not in picked, m.group(1)
            picked[m.group(1)] = b
    assert sorted(picked) == sorted(WANTED), sorted(picked)
    return "\n\n".join(picked[name] for name in WANTED)


def round_count(preset):
    text = open(os.path.join(REF, "configs", "constant_presets", preset + ".yaml")).read()
    return int(re.search(r"^SHUFFLE_ROUND_COUNT:\s*(\d+)", text, re.M).group(1))


def run_spec(code, rounds):
    ns = {"hash": lambda b: hashlib.sha256(b).digest(), "SHUFFLE_ROUND_COUNT": rounds,
          "ValidatorIndex": int, "Bytes32": bytes, "List": typing.List}
    exec(compile(code, SPEC, "exec"), ns)   # noqa: S102 -- the reference's own spec text
    return ns


def digest(values):
    return hashlib.sha256(struct.pack("<%dI" % len(values), *values)).hexdigest()


def main():
    code = pull_blocks()
    presets = {p: round_count(p) for p in ("minimal", "mainnet")}
    out = {"source": "specs/core/0_beacon-chain.md python blocks defining %s (fence rule of "
                     "scripts/function_puller.py:40-44)" % ", ".join(WANTED),
           "supplied": {"hash": "sha256", "SHUFFLE_ROUND_COUNT": presets,
                        "annotations": "ValidatorIndex=int, Bytes32=bytes, List=typing.List"},
           "cases_from": "test_generators/shuffling/main.py:18-20",
           "digest": "sha256 of the list packed as little-endian u32",
           "seeds": [], "cases": [], "committees": []}
    for preset, rounds in presets.items():
        ns = run_spec(code, rounds)
        seeds = [ns["hash"](ns["int_to_bytes"](k, length=4)) for k in range(N_SEEDS)]
        out["seeds"] = [s.hex() for s in seeds]
        for k, seed in enumerate(seeds):
            for count in COUNTS:
                shuffled = [ns["get_shuffled_index"](i, count, seed) for i in range(count)]
                case = {"preset": preset, "rounds": rounds, "seed": k, "count": count, "sha256": digest(shuffled)}
                if (k < 4 and count <= 100) or (k == 0 and count == 1000):
                    case["shuffled"] = shuffled
                out["cases"].append(case)
        indices = [(7 * i + 3) % 1000 + 5000 for i in range(1000)]   # a non-identity active set
        for committee_count in (3, 64):
            parts = [ns["compute_committee"](indices, seeds[0], j, committee_count) for j in range(committee_count)]
            out["committees"].append({"preset": preset, "rounds": rounds, "seed": 0,
                                      "indices": "(7 * i + 3) % 1000 + 5000 for i in range(1000)",
                                      "committee_count": committee_count, "lengths": [len(p) for p in parts],
                                      "sha256": digest([v for p in parts for v in p])})
        print(preset, rounds, "rounds:", len(out["cases"]), "cases so far", flush=True)
    with open(os.path.join(HERE, "shuffling.json"), "w") as f:
        f.write("{\n")
        keys = list(out)
        for key in keys:
            val = out[key]
            if key in ("cases", "committees"):
                f.write(' "%s": [\n' % key + ",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in val) + "\n ]")
            else:
                f.write(' "%s": %s' % (key, json.dumps(val)))
            f.write(",\n" if key != keys[-1] else "\n")
        f.write("}\n")
    print("shuffling.json:", len(out["cases"]), "cases,", len(out["committees"]), "committee splits")


if __name__ == "__main__":
    main()
