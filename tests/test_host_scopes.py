"""The scopes of the C-ABI host layer (consensus-specs_amd/csrc/bls381_scope.hpp), CPU only.

Fork, Held and the context's streams are written against the HIP types and a handful of runtime
calls; libbls381_hostcheck.so (test infrastructure, host_check.cpp) compiles them over stand-ins
that append to a call log, and hc_scope_scenario runs a named scenario and returns that log,
optionally with the k-th call after "begin" failing.  What every exit path queues is pinned here:
no GPU test forces a launch to fail.

Log lines: stream_create S / stream_destroy S / event_create E / event_destroy E / priority_range /
record E S / wait S E / sync S / launch S (work queued by the scenario) / FAIL <call> / released
<name> (held data destroyed) / complete (the parked events complete) and the scenario's own
"begin", "... rc N", "caught ...", "shutdown", "end".  S-1 is the caller's stream.
"""
import ctypes
import os
import subprocess

import pytest

MAIN = "S-1"


@pytest.fixture(scope="module")
def lib_path():
    import build_native
    return os.environ.get("BLS381_HOSTCHECK_LIB") or build_native.build_hostcheck()


@pytest.fixture(scope="module")
def run(lib_path):
    lib = ctypes.CDLL(lib_path)
    lib.hc_scope_scenario.restype = ctypes.c_long

    def scenario(name, fail_at=0):
        out = ctypes.create_string_buffer(1 << 16)
        n = lib.hc_scope_scenario(name.encode(), ctypes.c_int(fail_at), out, ctypes.c_size_t(len(out)))
        assert n >= 0, name
        return out.raw[:n].decode().splitlines()
    return scenario


def body(log):
    return log[log.index("begin") + 1:log.index("end")]


def created(log, what):
    return [ln.split()[1] for ln in log if ln.startswith(what + "_create ")]


def destroyed(log, what):
    return [ln.split()[1] for ln in log if ln.startswith(what + "_destroy ")]


def sides(log):
    """(stream, done event) of side, side2 and prio, and the fork event, from the creation order."""
    s, e = created(log, "stream"), created(log, "event")
    assert len(s) == 4 and len(e) == 4
    return list(zip(s[1:], e[:3])), e[3]


def joins_of(log, branched):
    """The join of `branched` side streams: per stream a record of its own event on it, then the
    main stream's wait on that event."""
    return [ln for st, ev in branched for ln in ("record %s %s" % (ev, st), "wait %s %s" % (MAIN, ev))]


def test_unknown_scenario_is_refused(lib_path):
    lib = ctypes.CDLL(lib_path)
    lib.hc_scope_scenario.restype = ctypes.c_long
    out = ctypes.create_string_buffer(64)
    assert lib.hc_scope_scenario(b"no such scenario", 0, out, ctypes.c_size_t(64)) == -1


def test_hostcheck_exports_no_runtime_name(lib_path):
    """The stand-ins and the scopes compiled over them have internal linkage: the library is loaded
    into processes that also hold the real runtime and the product library."""
    syms = subprocess.run(["nm", "-D", "--defined-only", lib_path], check=True, capture_output=True, text=True).stdout
    names = [ln.split()[-1] for ln in syms.splitlines() if ln.strip()]
    assert "hc_scope_scenario" in names
    bad = [n for n in names if n.lower().startswith("hip") or any(k in n for k in ("Fork", "Held", "KeepList", "Streams",
                                                                                  "streams_", "keep_until_done"))]
    assert not bad, bad


# ------------------------------------------------------------------------ Fork
def test_fork_normal_path(run):
    log = run("fork")
    (side, side2, _prio), fork_ev = sides(log)
    b = body(log)
    # one record on the main stream, of the fork event, after the work queued before the fork
    records_main = [ln for ln in b if ln.startswith("record ") and ln.endswith(" " + MAIN)]
    assert records_main == ["record %s %s" % (fork_ev, MAIN)]
    assert b.index("launch " + MAIN) < b.index(records_main[0])
    # each branched stream waits on it before anything else is logged for that stream
    for st, _ in (side, side2):
        mentions = [ln for ln in b if st in ln.split()]
        assert mentions[0] == "wait %s %s" % (st, fork_ev), mentions
        assert b.index(mentions[0]) > b.index(records_main[0])
    # the first join(): one record per branched stream on its own event, one wait of main per branch
    first = b.index("join rc 0")
    want = joins_of(log, [side, side2])
    assert b[first - len(want):first] == want
    assert [ln for ln in b if ln.startswith("record ")] == records_main + want[0::2]
    assert [ln for ln in b if ln.startswith("wait " + MAIN)] == want[1::2]
    # the side streams' work is queued before their records
    for st, ev in (side, side2):
        assert b.index("launch " + st) < b.index("record %s %s" % (ev, st))
    # a second join() logs nothing, and neither does the destructor
    assert b[first + 1:] == ["launch " + MAIN, "join rc 0", "pipeline rc 0"]
    assert not [ln for ln in b if ln.startswith("sync ")]


@pytest.mark.parametrize("name,tail", [("fork_return", "pipeline rc -2"), ("fork_throw", "caught workspace bound exceeded")])
def test_fork_scope_left_early_joins(run, name, tail):
    log, normal = run(name), run("fork")
    (side, side2, _prio), _ = sides(log)
    b = body(log)
    want = joins_of(log, [side, side2])
    assert want == joins_of(normal, sides(normal)[0][:2])   # the same joins as the normal path
    assert b[-1] == tail
    assert b[-1 - len(want):-1] == want
    nb = body(normal)
    assert b[:-1 - len(want)] == nb[:nb.index(want[0])]      # and the same calls before them


def test_fork_every_failing_call(run):
    """With the k-th record or wait failing, for each k: a failed branch is reported to the pipeline
    and what was branched is still joined; a failed join step leaves the remaining joins attempted,
    the side stream that could not be joined in stream order is waited for, and join() returns the
    first error."""
    normal = body(run("fork"))
    calls = [ln for ln in normal if ln.split()[0] in ("record", "wait")]
    assert len(calls) == 7   # fork record, 2 branch waits, 2 x (record + wait)
    for k in range(1, len(calls) + 1):
        log = run("fork", fail_at=k)
        (side, side2, _prio), fork_ev = sides(log)
        b = body(log)
        assert b.count("FAIL " + calls[k - 1]) == 1 and sum(ln.startswith("FAIL") for ln in b) == 1
        if k <= 3:   # the fork's record or a branch's wait: the pipeline returns its error
            assert b[-1] == "pipeline rc -1"
            branched = [] if k <= 2 else [side]
            want = joins_of(log, branched)
            after = b[b.index("FAIL " + calls[k - 1]) + 1:-1]
            assert after == want, (k, b)
            continue
        code = 1000 + k
        assert b.count("join rc %d" % code) == 2 and b[-1] == "pipeline rc 0"   # kept for the second join() too
        failed_side = side if k <= 5 else side2
        other = side2 if k <= 5 else side
        assert "sync " + failed_side[0] in b
        assert b.index("FAIL " + calls[k - 1]) < b.index("sync " + failed_side[0]) < b.index("join rc %d" % code)
        for ln in joins_of(log, [other]):   # the other branch is joined all the same
            assert ln in b and b.index(ln) < b.index("join rc %d" % code)
        assert "sync " + other[0] not in b


# ------------------------------------------------------------------------ Held
@pytest.mark.parametrize("name,rc", [("hold", 0), ("hold_return", -2)])
def test_held_data_outlives_the_scope_until_its_event_completes(run, name, rc):
    b = body(run(name))
    ev = created(b, "event")
    assert len(ev) == 3   # data, next, last
    entry = b.index("entry rc %d" % rc)
    # leaving the scope: an event recorded on the stream after the copy, nothing released
    assert b[entry - 2:entry] == ["event_create " + ev[0], "record %s %s" % (ev[0], MAIN)]
    assert "launch " + MAIN in b[:entry - 2]
    assert not [ln for ln in b[:entry] if ln.startswith("released")]
    # a later entry while the event is pending releases nothing; after completion the next one does
    done = b.index("complete")
    assert not [ln for ln in b[:done] if ln.startswith("released")]
    after = b[done + 1:b.index("shutdown")]
    assert after[:4] == ["event_destroy " + ev[0], "released data", "event_destroy " + ev[1], "released next"]
    # every created event is destroyed once, the last at shutdown
    assert sorted(destroyed(b, "event")) == sorted(ev)
    assert b[b.index("shutdown") + 1:] == ["event_destroy " + ev[2], "released last"]
    assert not [ln for ln in b if ln.startswith("sync ")]


@pytest.mark.parametrize("name", ["hold", "hold_return"])
@pytest.mark.parametrize("k,what", [(1, "event_create"), (2, "record")])
def test_held_data_without_an_event_waits_for_the_stream(run, name, k, what):
    b = body(run(name, fail_at=k))
    fail = [i for i, ln in enumerate(b) if ln.startswith("FAIL " + what)]
    assert len(fail) == 1
    i = fail[0]
    if what == "record":   # the event that could not be recorded is destroyed, then the stream waited for
        ev = b[i].split()[2]
        assert b[i + 1:i + 4] == ["event_destroy " + ev, "sync " + MAIN, "released data"]
    else:
        assert b[i + 1:i + 3] == ["sync " + MAIN, "released data"]
    assert sorted(destroyed(b, "event")) == sorted(created(b, "event"))
    assert b.count("released data") == b.count("released next") == b.count("released last") == 1


# ------------------------------------------------------- context create / destroy
def test_streams_full_create_and_destroy(run):
    b = body(run("streams"))
    assert "create rc 0" in b
    assert len(created(b, "stream")) == 4 and len(created(b, "event")) == 4
    for what in ("stream", "event"):
        assert sorted(destroyed(b, what)) == sorted(created(b, what))
    # a side stream is drained before it is destroyed
    for st in created(b, "stream")[1:]:
        assert b.index("sync " + st) < b.index("stream_destroy " + st)


def test_streams_every_failing_creation(run):
    n_calls = len([ln for ln in body(run("streams")) if ln.split()[0] in ("stream_create", "event_create", "priority_range")])
    assert n_calls == 9
    for k in range(1, n_calls + 1):
        b = body(run("streams", fail_at=k))
        assert "create rc %d" % (1000 + k) in b
        assert len(created(b, "stream")) + len(created(b, "event")) == (k - 1 if k <= 6 else k - 2)
        for what in ("stream", "event"):   # everything created before the failure is destroyed exactly once
            assert sorted(destroyed(b, what)) == sorted(created(b, what)), (k, b)
