"""CPU-side checks of the boundary: the C-ABI library loads and exports every
symbol include/bls381.h declares; the Python mirror keeps the reference's
module semantics (bls.py:3-46); with no device the product fails loudly (no
CPU fallback)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    txt = open(os.path.join(ROOT, "include", "bls381.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(bls381_\w+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    import build_native
    from bls381_amd import _native
    lib_path = build_native.build_hip()
    L = ctypes.CDLL(lib_path)
    names = header_functions()
    assert len(names) >= 20
    for n in names:
        assert hasattr(L, n), n
    assert sorted(_native._SIGS) == names, "ctypes binding table out of sync with include/bls381.h"
    _native.load_library()   # binds all signatures


def test_kernels_are_gfx950_code_objects():
    import build_native
    blob = open(build_native.build_hip(), "rb").read()
    # the offload bundle carries exactly one device target: gfx950
    assert b"hipv4-amdgcn-amd-amdhsa--gfx950" in blob
    assert b"amdhsa--gfx942" not in blob and b"amdhsa--gfx90a" not in blob


def test_no_device_fails_loudly():
    from bls381_amd import _native
    L = _native.load_library()
    if L.bls381_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(_native.NativeUnavailable):
        _native.lib()
    assert L.bls381_verify(b"\x00" * 48, b"\x00" * 32, 32, b"\x00" * 96, b"\x00" * 8) == _native.ENODEV


def test_stub_mode_mirrors_reference():
    from bls381_amd import bls
    assert bls.STUB_SIGNATURE == b"\x11" * 96 and bls.STUB_PUBKEY == b"\x22" * 48
    old = bls.bls_active
    try:
        bls.bls_active = False
        assert bls.bls_verify(b"", b"", b"", 0) is True
        assert bls.bls_verify_multiple([], [], b"", 0) is True
        assert bls.bls_aggregate_pubkeys([b"x"]) == bls.STUB_PUBKEY
        assert bls.bls_aggregate_signatures([]) == bls.STUB_SIGNATURE
        assert bls.bls_sign(b"m", 1, 0) == bls.STUB_SIGNATURE
    finally:
        bls.bls_active = old


def test_errors_raised_before_the_engine():
    from bls381_amd import bls
    with pytest.raises(ValueError):
        bls.bls_verify_multiple([b"\x00" * 48], [], b"\x00" * 96, 0)
    with pytest.raises(bls.ValidationError):
        bls.bls_verify_multiple([], [b"\x00" * 32], b"\x00" * 96, 0)
    # the strict policy takes the spec's types: a uint64 domain, checked first, and Bytes48 /
    # Bytes96 (other lengths are invalid inputs -> False without reaching the device).  Under
    # the py_ecc policy both need the engine (py_ecc decodes before it serialises the domain,
    # and reads other lengths as integers): tests/test_gpu_parity.py::test_shim_lengths_and_domain_order
    old = bls.SUBGROUP_POLICY
    bls.SUBGROUP_POLICY = "strict"
    try:
        with pytest.raises(OverflowError):
            bls.bls_verify(b"\x00" * 48, b"\x00" * 32, b"\x00" * 96, 2 ** 64)
        with pytest.raises(OverflowError):
            bls.bls_verify(b"\x00" * 48, b"\x00" * 32, b"\x00" * 96, -1)
        with pytest.raises(OverflowError):
            bls.bls_verify_multiple([], [], b"\x00" * 96, 2 ** 64)
        assert bls.bls_verify(b"\x00" * 47, b"\x00" * 32, b"\x00" * 96, 0) is False
        with pytest.raises(ValueError):
            bls.bls_aggregate_pubkeys([b"\x00" * 47])
    finally:
        bls.SUBGROUP_POLICY = old


def test_keyword_names_match_reference():
    import inspect
    from bls381_amd import bls
    # reference bls.py:25,30,35,40,45 (callers pass kwargs, 0_beacon-chain.md:1024-1033)
    want = {"bls_verify": ["pubkey", "message_hash", "signature", "domain"],
            "bls_verify_multiple": ["pubkeys", "message_hashes", "signature", "domain"],
            "bls_aggregate_pubkeys": ["pubkeys"],
            "bls_aggregate_signatures": ["signatures"],
            "bls_sign": ["message_hash", "privkey", "domain"]}
    for name, params in want.items():
        fn = getattr(bls, name)
        inner = next(c.cell_contents for c in fn.__closure__ if callable(c.cell_contents))
        assert list(inspect.signature(inner).parameters) == params, name


def test_registry_shim_hook_is_opt_in():
    from bls381_amd import bls
    assert bls._pubkey_registry is None
    bls.use_pubkey_registry(None)
    assert bls._pubkey_registry is None


def test_message_longer_than_limit_raises():
    """The one divergence from py_ecc's bool-only verify contract (bls.py header): a message
    over _native.MSG_MAX raises ValueError before any engine call."""
    from bls381_amd import _native, bls
    big = b"\x00" * (_native.MSG_MAX + 1)
    with pytest.raises(ValueError):
        bls.bls_verify(b"\x00" * 48, big, b"\x00" * 96, 0)
    with pytest.raises(ValueError):
        bls.bls_verify_multiple([b"\x00" * 48], [big], b"\x00" * 96, 0)
    with pytest.raises(ValueError):
        bls.bls_sign(big, 1, 0)


def test_thread_policy_override_is_per_thread():
    """bls381_set_thread_subgroup_policy: a thread's override never changes the
    process-wide policy other threads and front ends read, and -1 clears it."""
    import threading
    from bls381_amd import _native
    _native.set_subgroup_policy("strict")
    try:
        seen = {}
        with _native.subgroup_policy_scope("pyecc"):
            assert _native.get_thread_subgroup_policy() == "pyecc"
            assert _native.get_subgroup_policy() == "strict"
            t = threading.Thread(target=lambda: seen.setdefault("other", _native.get_thread_subgroup_policy()))
            t.start()
            t.join()
            with _native.subgroup_policy_scope("strict"):
                assert _native.get_thread_subgroup_policy() == "strict"
            assert _native.get_thread_subgroup_policy() == "pyecc"   # nested scope restored
        assert seen["other"] == "strict"
        assert _native.get_thread_subgroup_policy() == "strict"      # override cleared
        L = _native.load_library()
        assert L.bls381_set_thread_subgroup_policy(7) == _native.EARG
    finally:
        _native.set_subgroup_policy("pyecc")


def test_shim_does_not_rewrite_process_policy():
    """bls.bls_verify scopes its policy to the call: the shim's own 'strict' does not leak into
    the process-wide policy (a call that stops before the device: a wrong length under the
    shim's strict policy).  The converse -- a process-wide 'strict' surviving a shim call that
    reaches the device -- is tests/test_gpu_parity.py::test_shim_call_keeps_process_policy."""
    from bls381_amd import _native, bls
    old = bls.SUBGROUP_POLICY
    bls.SUBGROUP_POLICY = "strict"
    try:
        assert bls.bls_verify(b"\x00" * 47, b"\x00" * 32, b"\x00" * 96, 0) is False
        assert _native.get_subgroup_policy() == "pyecc"
    finally:
        bls.SUBGROUP_POLICY = old


def test_rccl_path_resolves_without_a_device():
    """bls381_comm_rccl_path: the RCCL the communicator would use (dlopen only, no device);
    bench.py records it next to the librccl objects mapped in the process."""
    from bls381_amd import comm
    try:
        p = comm.rccl_path()
    except Exception as e:   # an image without RCCL: the native multi-GPU path is unavailable
        pytest.skip("RCCL not loadable: %s" % e)
    assert "rccl" in os.path.basename(p)
    assert os.path.realpath(p) in comm.loaded_rccl_paths()


@pytest.mark.parametrize("libname", ["libbls381.so", "libbls381_devcheck.so"])
def test_library_has_no_flat_instructions(libname):
    """VERDICT r05 weak #6 / DESIGN.md section 10.8: no generic (flat) memory access in the shipped
    gfx950 code object.  Round 5 removed every pointer into a caller's private memory from the
    call boundaries (by-value operands, force-inlined reference helpers, address_space(1) SoA
    accessors): a flat access to the private aperture is the fault class of the round-2 max-ilp
    and round-5 BLS_FP2_INLINE=2 builds.  Static check of lib/libbls381.so, and of the device check
    library lib/libbls381_devcheck.so, whose probes follow the same discipline (no GPU)."""
    import subprocess
    import sys
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    so = os.path.join(ROOT, "consensus-specs_amd", "lib", libname)
    if not os.path.exists(objdump) or not os.path.exists(so):
        pytest.skip("llvm-objdump or the built library missing")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from extract_co import extract
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        co = os.path.join(d, "bls.co")
        extract(so, co)
        dis = subprocess.run([objdump, "-d", "--no-show-raw-insn", co], capture_output=True, text=True,
                             timeout=300).stdout
    flat = [ln.strip() for ln in dis.splitlines() if ln.strip().startswith("flat_")]
    assert "v_mad_u64_u32" in dis          # the disassembly is the engine's
    assert not flat, "%d flat instructions, e.g. %s" % (len(flat), flat[:3])
