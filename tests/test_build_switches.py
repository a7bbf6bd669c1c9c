"""The build and run-time switches of the native sources against DESIGN.md's table of them
(§0, "Build switches"): every `#ifndef BLS_... / #define` default in csrc/*.hpp and
bls381_capi.hip and every name read through env_knob(...) has a row, every row has a definition,
and the decided A/B switches that were removed stay removed.  A forgotten measurement switch fails
here instead of waiting for a review.
"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "consensus-specs_amd", "csrc")

REMOVED = ["BLS_ML_LINES_LDS", "BLS_ML_ACCUM_LDS", "BLS_ML_L_NT", "BLS_HASH_COMPACT", "BLS_WAVE_BALANCE",
           "BLS_INV_PAIR", "BLS_POW_PAIR", "BLS_LAZY_CSQR", "BLS_LAZY_CSQR_V2", "BLS_ML_QUAD_INLINE",
           "BLS_BP_INLINE_LADDERS"]

TABLE_HEAD = "| switch | kind | default | defined in | non-default side run by |"


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _source_switches():
    names = set()
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hpp"))) + [os.path.join(CSRC, "bls381_capi.hip")]:
        text = _read(path)
        # a default: #ifndef NAME directly followed by #define NAME
        names.update(m.group(1) for m in re.finditer(
            r"^[ \t]*#[ \t]*ifndef[ \t]+(BLS_\w+)[^\n]*\n[ \t]*#[ \t]*define[ \t]+\1\b", text, re.M))
        names.update(re.findall(r"\benv_knob\(\s*\"(\w+)\"", text))
    return names


def _design_table():
    lines = _read(os.path.join(ROOT, "DESIGN.md")).splitlines()
    starts = [i for i, ln in enumerate(lines) if ln.strip() == TABLE_HEAD]
    assert len(starts) == 1, "DESIGN.md holds the switch table exactly once"
    rows = {}
    for ln in lines[starts[0] + 2:]:
        cells = [c.strip() for c in ln.strip().strip("|").split("|")]
        if not ln.strip().startswith("|"):
            break
        assert len(cells) == 5, ln
        name = cells[0].strip("`")
        assert name not in rows, name
        rows[name] = cells
    return rows


def test_design_table_lists_exactly_the_switches_in_the_sources():
    src, rows = _source_switches(), _design_table()
    assert len(src) > 10 and "BLS381_FE_OCT" in src and "BLS_WAVES_PER_EU" in src   # the scan finds them
    assert set(rows) == src, (sorted(src - set(rows)), sorted(set(rows) - src))
    for name, cells in rows.items():
        assert cells[1] in ("build parameter", "hook", "environment knob"), cells
        assert cells[1] == "environment knob" if name.startswith("BLS381_") else cells[1] != "environment knob", cells
        # the file named holds the definition
        text = _read(os.path.join(CSRC, cells[3].strip("`")))
        assert re.search(r"#[ \t]*define[ \t]+%s\b|env_knob\(\s*\"%s\"" % (name, name), text), cells


def test_removed_switches_stay_removed():
    files = []
    for top, _, fs in os.walk(os.path.join(ROOT, "consensus-specs_amd")):
        if os.path.basename(top) in ("lib", "__pycache__"):
            continue
        files += [os.path.join(top, f) for f in fs if f.endswith((".hpp", ".hip", ".cpp", ".py", ".h"))]
    files += glob.glob(os.path.join(ROOT, "tools", "*.hip")) + glob.glob(os.path.join(ROOT, "tools", "*.py"))
    assert len(files) > 30
    pat = re.compile(r"\b(%s)\b" % "|".join(REMOVED))
    hits = [(os.path.relpath(p, ROOT), m.group(1)) for p in files for m in pat.finditer(_read(p))]
    assert not hits, hits
