"""SSZ hash_tree_root / signing_root of fixed-size containers on the GPU -- the
message_hash producer in front of bls_verify.

The reference computes every BLS message with SSZ merkleization on the CPU:
``signing_root(deposit.data)`` for deposits (specs/core/0_beacon-chain.md:1755-1758)
and ``hash_tree_root(AttestationDataAndCustodyBit(...))`` for attestations
(:1029-1030), through test_libs/pyspec/eth2spec/utils/ssz/ssz_impl.py:143-163.
Here a fixed-size type compiles into a short program over the item's SSZ
serialization (csrc/bls381_ssz.hpp), and the engine runs it for a whole batch,
one lane per item.  The bytes equal ssz_impl's for the same values.

Types: ``uint(nbytes)``, ``BOOL``, ``Bytes(n)``, ``Vector(type, n)``,
``Container((name, type), ...)``; the beacon-chain containers on the BLS path are
predefined below.

``verify_merkle_branch_batch`` runs the spec's verify_merkle_branch
(0_beacon-chain.md:846-857) for a batch; the whole of process_deposit is
``registry.PubkeyRegistry.process_deposits``.

Across items (csrc/bls381_merkle.hpp): ``merkle_root`` and ``merkle_proofs`` are the reference's
utils/merkle_minimal.py trees (zero-padded to 2**depth leaves, the given ones from index
``first``), ``build_deposits`` turns DepositData into Deposits with their proofs under one
root.  ``hash_tree_root(typ, value)`` and ``signing_root(typ, value)`` take Python values of any
type below, ``List(elem)`` and ``BYTES`` (the spec's ``bytes``) included.

Variable-size containers (csrc/bls381_ssz.hpp ``ssz_run_ragged``): a container whose
variable-size fields are lists of basic elements or such containers again -- ``PendingAttestation``,
``Attestation``, ``IndexedAttestation``, ``AttesterSlashing`` -- compiles into a ragged program that
follows the offsets of its serialization, so ``hash_tree_root_ragged_batch`` and ``list_root_ragged``
take a whole batch of them in one call, and ``hash_tree_root`` of a list of them is one call too.
Serialized items are untrusted: one that breaks the offset rules gets status 1 and a zero root.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native

SSZ_CHUNK = 1
SSZ_MERKLE = 2
# the ops of a ragged program (csrc/bls381_defs.hpp)
SSZ_RAGGED = 3
SSZ_FIELD = 4
SSZ_ENTER = 5
SSZ_LEAVE = 6
SSZ_NO_NEXT = 0xFFFFFFFF
SSZ_SCOPE_MAX = 4
SSZ_FIXED_MAX = 1 << 16
BYTES_PER_LENGTH_OFFSET = 4


def uint(n: int):
    return ("uint", n)


BOOL = ("bool",)


def Bytes(n: int):
    return ("bytes", n)


def Vector(elem, n: int):
    return ("vector", elem, n)


def List(elem):
    return ("list", elem)


def Container(*fields):
    return ("container", list(fields))


BYTES = List(uint(1))      # the spec's `bytes`; values may be bytes objects


# specs/core/0_beacon-chain.md containers whose roots are BLS messages
Crosslink = Container(("shard", uint(8)), ("start_epoch", uint(8)), ("end_epoch", uint(8)),
                      ("parent_root", Bytes(32)), ("data_root", Bytes(32)))
AttestationData = Container(("beacon_block_root", Bytes(32)), ("source_epoch", uint(8)),
                            ("source_root", Bytes(32)), ("target_epoch", uint(8)), ("target_root", Bytes(32)),
                            ("crosslink", Crosslink))
AttestationDataAndCustodyBit = Container(("data", AttestationData), ("custody_bit", BOOL))
DepositData = Container(("pubkey", Bytes(48)), ("withdrawal_credentials", Bytes(32)), ("amount", uint(8)),
                        ("signature", Bytes(96)))
Deposit = Container(("proof", Vector(Bytes(32), 32)), ("data", DepositData))
BeaconBlockHeader = Container(("slot", uint(8)), ("parent_root", Bytes(32)), ("state_root", Bytes(32)),
                              ("body_root", Bytes(32)), ("signature", Bytes(96)))

# further containers of 0_beacon-chain.md: the elements of BeaconState's and BeaconBlockBody's lists
Fork = Container(("previous_version", Bytes(4)), ("current_version", Bytes(4)), ("epoch", uint(8)))
Validator = Container(("pubkey", Bytes(48)), ("withdrawal_credentials", Bytes(32)),
                      ("activation_eligibility_epoch", uint(8)), ("activation_epoch", uint(8)),
                      ("exit_epoch", uint(8)), ("withdrawable_epoch", uint(8)), ("slashed", BOOL),
                      ("effective_balance", uint(8)))
Eth1Data = Container(("deposit_root", Bytes(32)), ("deposit_count", uint(8)), ("block_hash", Bytes(32)))
ProposerSlashing = Container(("proposer_index", uint(8)), ("header_1", BeaconBlockHeader),
                             ("header_2", BeaconBlockHeader))
VoluntaryExit = Container(("epoch", uint(8)), ("validator_index", uint(8)), ("signature", Bytes(96)))
Transfer = Container(("sender", uint(8)), ("recipient", uint(8)), ("amount", uint(8)), ("fee", uint(8)),
                     ("slot", uint(8)), ("pubkey", Bytes(48)), ("signature", Bytes(96)))

# the variable-size containers of 0_beacon-chain.md:345-523 and the block around them
IndexedAttestation = Container(("custody_bit_0_indices", List(uint(8))), ("custody_bit_1_indices", List(uint(8))),
                               ("data", AttestationData), ("signature", Bytes(96)))
PendingAttestation = Container(("aggregation_bitfield", BYTES), ("data", AttestationData),
                               ("inclusion_delay", uint(8)), ("proposer_index", uint(8)))
AttesterSlashing = Container(("attestation_1", IndexedAttestation), ("attestation_2", IndexedAttestation))
Attestation = Container(("aggregation_bitfield", BYTES), ("data", AttestationData), ("custody_bitfield", BYTES),
                        ("signature", Bytes(96)))
BeaconBlockBody = Container(("randao_reveal", Bytes(96)), ("eth1_data", Eth1Data), ("graffiti", Bytes(32)),
                            ("proposer_slashings", List(ProposerSlashing)),
                            ("attester_slashings", List(AttesterSlashing)), ("attestations", List(Attestation)),
                            ("deposits", List(Deposit)), ("voluntary_exits", List(VoluntaryExit)),
                            ("transfers", List(Transfer)))
BeaconBlock = Container(("slot", uint(8)), ("parent_root", Bytes(32)), ("state_root", Bytes(32)),
                        ("body", BeaconBlockBody), ("signature", Bytes(96)))


def is_fixed_size(typ) -> bool:
    """ssz_impl.py:43-53."""
    k = typ[0]
    if k == "list":
        return False
    if k == "vector":
        return is_fixed_size(typ[1])
    if k == "container":
        return all(is_fixed_size(t) for _, t in typ[1])
    return True


def item_size(typ) -> int:
    k = typ[0]
    if k == "uint":
        return typ[1]
    if k == "bool":
        return 1
    if k == "bytes":
        return typ[1]
    if k == "vector":
        return typ[2] * item_size(typ[1])
    return sum(item_size(t) for _, t in typ[1])


def _encode_series(types, values) -> bytes:
    """ssz_impl.py:72-103: the fixed parts in order, a 4-byte offset in place of each variable-size
    part, then the variable parts."""
    parts = [(is_fixed_size(t), serialize(t, x)) for t, x in zip(types, values)]
    offset = sum(len(p) if fixed else BYTES_PER_LENGTH_OFFSET for fixed, p in parts)
    if offset + sum(len(p) for fixed, p in parts if not fixed) >= 1 << (8 * BYTES_PER_LENGTH_OFFSET):
        raise ValueError("the serialization does not fit 32-bit offsets")
    head, tail = [], []
    for fixed, p in parts:
        if fixed:
            head.append(p)
        else:
            head.append(offset.to_bytes(BYTES_PER_LENGTH_OFFSET, "little"))
            tail.append(p)
            offset += len(p)
    return b"".join(head + tail)


def serialize(typ, v) -> bytes:
    """SSZ serialization (ssz_impl.py:21-30 for basics, :60-103 for series and containers)."""
    k = typ[0]
    if k == "uint":
        return int(v).to_bytes(typ[1], "little")
    if k == "bool":
        return b"\x01" if v else b"\x00"
    if k == "bytes":
        v = bytes(v)
        if len(v) != typ[1]:
            raise ValueError("expected %d bytes" % typ[1])
        return v
    if k in ("vector", "list"):
        if k == "vector" and len(v) != typ[2]:
            raise ValueError("expected %d elements" % typ[2])
        if isinstance(v, (bytes, bytearray)) and typ[1] == uint(1):
            return bytes(v)
        return _encode_series([typ[1]] * len(v), list(v))
    return _encode_series([t for _, t in typ[1]], [v[name] for name, _ in typ[1]])


def _emit(typ, off: int, prog: list) -> int:
    k = typ[0]
    if k in ("uint", "bool"):
        n = item_size(typ)
        prog += [SSZ_CHUNK, off, n]
        return off + n
    if k == "bytes":
        n = typ[1]
        pieces = max(1, (n + 31) // 32)
        for j in range(pieces):
            prog += [SSZ_CHUNK, off + 32 * j, min(32, n - 32 * j)]
        if pieces > 1:
            prog += [SSZ_MERKLE, pieces]
        return off + n
    if k == "vector":
        if typ[1][0] in ("uint", "bool"):
            # basic elements are packed (ssz_impl.py:110-123): the chunks of the serialization
            return _emit(Bytes(item_size(typ)), off, prog)
        for _ in range(typ[2]):
            off = _emit(typ[1], off, prog)
        prog += [SSZ_MERKLE, typ[2]]
        return off
    for _, t in typ[1]:
        off = _emit(t, off, prog)
    prog += [SSZ_MERKLE, len(typ[1])]
    return off


def fixed_part_size(typ) -> int:
    """Bytes of a container's fixed part: its fixed-size fields and an offset word per variable one."""
    return sum(item_size(t) if is_fixed_size(t) else BYTES_PER_LENGTH_OFFSET for _, t in typ[1])


def _emit_scope(typ, count: int, prog: list) -> None:
    """The ops over one scope of a ragged program: the first `count` fields of the container."""
    pos, off = [], 0
    for _, t in typ[1]:
        pos.append(off)
        off += item_size(t) if is_fixed_size(t) else BYTES_PER_LENGTH_OFFSET
    var = [i for i, (_, t) in enumerate(typ[1]) if not is_fixed_size(t)]
    for i, (_, t) in enumerate(typ[1][:count]):
        if is_fixed_size(t):
            _emit(t, pos[i], prog)
            continue
        later = [pos[j] for j in var if j > i]
        nxt = later[0] if later else SSZ_NO_NEXT
        if t[0] == "list" and t[1][0] in ("uint", "bool"):
            prog += [SSZ_FIELD, pos[i], nxt, item_size(t[1])]
        elif t[0] == "container":
            prog += [SSZ_ENTER, pos[i], nxt, fixed_part_size(t)]
            _emit_scope(t, len(t[1]), prog)
            prog += [SSZ_LEAVE]
        else:
            raise ValueError("a ragged program takes lists of basic elements and containers of them")
    prog += [SSZ_MERKLE, count]


def compile_root(typ, signing: bool = False) -> np.ndarray:
    """The root program of `typ` (signing=True: signing_root, the last field left out).  A
    variable-size container gives a ragged program; ValueError when a variable-size field of it
    is neither a list of basic elements nor such a container."""
    prog: list = []
    if signing and (typ[0] != "container" or len(typ[1]) < 2):
        raise ValueError("signing_root needs a container with at least two fields")
    if typ[0] == "container" and not is_fixed_size(typ):
        prog += [SSZ_RAGGED, fixed_part_size(typ)]
        _emit_scope(typ, len(typ[1]) - (1 if signing else 0), prog)
    elif not is_fixed_size(typ):
        raise ValueError("a root program takes a fixed-size type or a variable-size container")
    elif signing:
        off = 0
        for _, t in typ[1][:-1]:
            off = _emit(t, off, prog)
        prog += [SSZ_MERKLE, len(typ[1]) - 1]
    else:
        _emit(typ, 0, prog)
    return np.asarray(prog, dtype=np.uint32)


def _roots(typ, items, signing: bool) -> list:
    size = item_size(typ)
    blob = b"".join(bytes(x) for x in items)
    n = len(blob) // size
    if n * size != len(blob):
        raise ValueError("items must be %d-byte serializations" % size)
    if n == 0:
        return []
    prog = compile_root(typ, signing)
    out = ctypes.create_string_buffer(32 * n)
    _native.check(_native.lib().bls381_ssz_root_batch(n, blob, size, prog.ctypes.data_as(ctypes.c_void_p),
                                                      len(prog), out))
    raw = out.raw
    return [raw[32 * i:32 * i + 32] for i in range(n)]


def hash_tree_root_batch(typ, serialized_items) -> list:
    """hash_tree_root of each serialized item (ssz_impl.py:143-155)."""
    return _roots(typ, serialized_items, False)


def signing_root_batch(typ, serialized_items) -> list:
    """signing_root of each serialized container (ssz_impl.py:158-163)."""
    return _roots(typ, serialized_items, True)


def ragged_prog_ok(prog, max_field_bytes: int = 0) -> bool:
    """csrc/bls381_plan.hpp ssz_ragged_prog_ok: the walk the engine makes before it runs a ragged
    program (max_field_bytes 0: the longest field a 32-bit offset admits)."""
    prog = [int(x) for x in prog]
    n = len(prog)
    if n < 2 or n > SSZ_PROG_MAX or prog[0] != SSZ_RAGGED or prog[1] > SSZ_FIXED_MAX:
        return False
    if max_field_bytes <= 0 or max_field_bytes > 0xFFFFFFFF:
        max_field_bytes = 0xFFFFFFFF
    stream = chunk_depth((max_field_bytes + 31) // 32) + 1
    fixed, sp, peak, pc = [prog[1]], 0, 0, 2
    while pc < n:
        op = prog[pc]
        if op == SSZ_CHUNK and pc + 2 < n:
            if prog[pc + 2] > 32 or prog[pc + 1] + prog[pc + 2] > fixed[-1]:
                return False
            sp, pc = sp + 1, pc + 3
        elif op == SSZ_MERKLE and pc + 1 < n:
            k = prog[pc + 1]
            if k == 0 or k > sp:
                return False
            peak = max(peak, sp - k + (1 << chunk_depth(k)))
            sp, pc = sp - k + 1, pc + 2
        elif op in (SSZ_FIELD, SSZ_ENTER) and pc + 3 < n:
            pos, nxt, arg = prog[pc + 1:pc + 4]
            if pos + 4 > fixed[-1] or (nxt != SSZ_NO_NEXT and nxt + 4 > fixed[-1]):
                return False
            if op == SSZ_FIELD:
                if arg not in (1, 2, 4, 8, 16, 32):
                    return False
                peak = max(peak, sp + stream)
                sp += 1
            else:
                if len(fixed) >= SSZ_SCOPE_MAX or arg > SSZ_FIXED_MAX:
                    return False
                fixed.append(arg)
            pc += 4
        elif op == SSZ_LEAVE:
            if len(fixed) == 1:
                return False
            fixed.pop()
            pc += 1
        else:
            return False
        peak = max(peak, sp)
    return sp == 1 and len(fixed) == 1 and peak <= SSZ_STACK


def _ragged_fits(typ) -> bool:
    """Whether `typ` is a variable-size container that one lane roots from its serialization."""
    if typ[0] != "container" or is_fixed_size(typ):
        return False
    try:
        return ragged_prog_ok(compile_root(typ))
    except ValueError:
        return False


def _ragged_args(typ, serialized_items):
    items = [bytes(x) for x in serialized_items]
    prog = compile_root(typ)
    if is_fixed_size(typ) or not ragged_prog_ok(prog):
        raise ValueError("not a type with a ragged root program")
    starts = np.zeros(len(items) + 1, dtype=np.uint64)
    np.cumsum([len(x) for x in items], out=starts[1:])
    return items, b"".join(items), starts, prog


def hash_tree_root_ragged_batch(typ, serialized_items):
    """(roots, status): hash_tree_root of each serialized variable-size container, in one call.  A
    serialization that breaks the offset rules has status 1 and a zero root."""
    items, blob, starts, prog = _ragged_args(typ, serialized_items)
    n = len(items)
    status = np.zeros(n, dtype=np.uint8)
    if n == 0:
        return [], status
    out = ctypes.create_string_buffer(32 * n)
    _native.check(_native.lib().bls381_ssz_ragged_roots(n, blob or None, starts.ctypes.data_as(ctypes.c_void_p),
                                                        prog.ctypes.data_as(ctypes.c_void_p), len(prog), out,
                                                        status.ctypes.data_as(ctypes.c_void_p)))
    raw = out.raw
    return [raw[32 * i:32 * i + 32] for i in range(n)], status


def list_root_ragged(typ, serialized_items, mix_length: bool = True) -> bytes:
    """hash_tree_root of the list of the serialized variable-size containers, in one call;
    ValueError when one of them breaks the offset rules."""
    items, blob, starts, prog = _ragged_args(typ, serialized_items)
    out = ctypes.create_string_buffer(32)
    _native.check(_native.lib().bls381_ssz_ragged_list_root(
        len(items), blob or None, starts.ctypes.data_as(ctypes.c_void_p), prog.ctypes.data_as(ctypes.c_void_p),
        len(prog), int(bool(mix_length)), out, None))
    return out.raw


def verify_deposits(deposit_datas, domain) -> np.ndarray:
    """process_deposit's check for each serialized DepositData (0_beacon-chain.md:1755-1758):
    bls_verify(pubkey, signing_root(deposit.data), signature, domain), roots computed on the device."""
    blob = b"".join(bytes(x) for x in deposit_datas)
    n = len(blob) // 184
    if n * 184 != len(blob):
        raise ValueError("DepositData serializations are 184 bytes")
    out = np.zeros(n, dtype=np.uint8)
    if n:
        dom = int(domain).to_bytes(8, "big") * n
        _native.check(_native.lib().bls381_verify_deposits(n, blob, dom, out.ctypes.data_as(ctypes.c_void_p)))
    return out.astype(bool)


def verify_merkle_branch_batch(leaves, proofs, depth: int, indices, root_or_roots) -> np.ndarray:
    """verify_merkle_branch (0_beacon-chain.md:846-857) per item: ``leaves[i]`` (32 bytes) with the
    ``depth`` siblings ``proofs[i]`` (a sequence of 32-byte values, or their concatenation) under
    ``indices[i]`` against one 32-byte root, or against ``root_or_roots[i]``."""
    leaves = [bytes(x) for x in leaves]
    n = len(leaves)
    depth = int(depth)
    flat = [bytes(p) if isinstance(p, (bytes, bytearray, memoryview)) else b"".join(bytes(s) for s in p)
            for p in proofs]
    single = isinstance(root_or_roots, (bytes, bytearray, memoryview))
    roots = [bytes(root_or_roots)] if single else [bytes(r) for r in root_or_roots]
    idx = np.ascontiguousarray([int(i) for i in indices], dtype=np.uint64)
    if (any(len(x) != 32 for x in leaves) or any(len(r) != 32 for r in roots) or len(flat) != n or len(idx) != n
            or any(len(p) != 32 * depth for p in flat) or (not single and len(roots) != n)):
        raise ValueError("verify_merkle_branch_batch: 32-byte leaves and roots, depth siblings and one index per item")
    out = np.zeros(n, dtype=np.uint8)
    # depth and the stride are checked by the engine (BLS381_EARG -> ValueError)
    _native.check(_native.lib().bls381_merkle_branch_batch(
        n, b"".join(leaves) or None, b"".join(flat) or None, depth, idx.ctypes.data_as(ctypes.c_void_p) if n else None,
        b"".join(roots) or None, 0 if single else 32, out.ctypes.data_as(ctypes.c_void_p) if n else None))
    return out.astype(bool)


# ---------------------------------------------------------------- trees across items
def _leaf_blob(leaves) -> bytes:
    blob = bytes(leaves) if isinstance(leaves, (bytes, bytearray, memoryview)) else b"".join(bytes(x) for x in leaves)
    if len(blob) % 32:
        raise ValueError("leaves are 32 bytes each")
    return blob


def chunk_depth(n: int) -> int:
    """Depth of merkleize_chunks over n chunks (merkle_minimal.py): ceil(log2 n), 0 for n <= 1."""
    return 0 if n <= 1 else (n - 1).bit_length()


def merkle_root(leaves, depth: int, first: int = 0, length=None) -> bytes:
    """Root of the tree with 2**depth leaves of which ``first .. first+n-1`` are ``leaves`` (32-byte
    values, or their concatenation) and the others zero: get_merkle_root is depth 32,
    merkleize_chunks depth ceil(log2 n).  No leaves give the zero node of ``depth``.  With
    ``length`` the root is mixed with it (mix_in_length, ssz_impl.py:122-124)."""
    blob = _leaf_blob(leaves)
    out = ctypes.create_string_buffer(32)
    _native.check(_native.lib().bls381_merkle_root(len(blob) // 32, blob or None, int(first), int(depth),
                                                   0 if length is None else 1, 0 if length is None else int(length),
                                                   out))
    return out.raw


def merkle_proofs(leaves, depth: int, indices, first: int = 0):
    """get_merkle_proof of the same tree for each of ``indices`` (leaf indices below 2**depth; one
    outside the window gets the proof of a zero leaf).  Returns (proofs, root): proofs[k] is the
    concatenation of the ``depth`` siblings of indices[k], the form verify_merkle_branch_batch takes."""
    blob = _leaf_blob(leaves)
    depth = int(depth)
    idx = np.ascontiguousarray([int(i) for i in indices], dtype=np.uint64)
    if any(int(i) >> depth for i in idx):
        raise ValueError("merkle_proofs: an index at or above 2**depth")
    row = 32 * depth
    out = ctypes.create_string_buffer(max(row * len(idx), 1))
    root = ctypes.create_string_buffer(32)
    _native.check(_native.lib().bls381_merkle_proofs(len(blob) // 32, blob or None, int(first), depth, len(idx),
                                                     idx.ctypes.data_as(ctypes.c_void_p) if len(idx) else None, out,
                                                     row, root))
    raw = out.raw
    return [raw[row * k:row * k + row] for k in range(len(idx))], root.raw


def build_deposits(deposit_datas, first_index: int = 0):
    """Serialized Deposits (1,208 bytes: the proof, then the data) for serialized DepositData
    (184 bytes each) that sit at leaves ``first_index ..`` of the deposit tree, and the tree's root:
    what test/helpers/deposits.py of the reference builds with merkle_minimal.py, and what
    ``PubkeyRegistry.process_deposits(deposits, first_index, root, ...)`` consumes."""
    blob = b"".join(bytes(x) for x in deposit_datas)
    n = len(blob) // 184
    if n * 184 != len(blob):
        raise ValueError("DepositData serializations are 184 bytes")
    out = ctypes.create_string_buffer(max(1208 * n, 1))
    root = ctypes.create_string_buffer(32)
    _native.check(_native.lib().bls381_deposits_build(n, blob or None, int(first_index), out, root))
    raw = out.raw
    return [raw[1208 * i:1208 * i + 1208] for i in range(n)], root.raw


SSZ_STACK = 64        # csrc/bls381_defs.hpp: chunks of a root program's stack
SSZ_PROG_MAX = 512    # and its length in words


def _program_fits(typ, signing: bool = False) -> bool:
    """Whether one lane can run the type's root program (bls381_plan.hpp ssz_prog_ok's bounds)."""
    if not is_fixed_size(typ):
        return False
    chunks = _peak_chunks(typ, signing)
    return chunks is not None and len(compile_root(typ, signing)) <= SSZ_PROG_MAX


def _peak_chunks(typ, signing: bool = False):
    """The stack peak of the root program in chunks, or None above SSZ_STACK (found without
    emitting the program of a large vector)."""
    def peak(t, below):
        # returns the peak while t's root is computed with `below` chunks under it, or None
        k = t[0]
        if k in ("uint", "bool"):
            return below + 1
        if k == "bytes" or (k == "vector" and t[1][0] in ("uint", "bool")):
            pieces = max(1, (item_size(t) + 31) // 32)
            return below + (1 << chunk_depth(pieces))
        parts = [t[1]] * t[2] if k == "vector" else [ft for _, ft in t[1]]
        if len(parts) + below > SSZ_STACK:
            return None
        top = below
        for j, ft in enumerate(parts):
            p = peak(ft, below + j)
            if p is None:
                return None
            top = max(top, p)
        return max(top, below + (1 << chunk_depth(len(parts))))
    t = Container(*typ[1][:-1]) if signing else typ
    p = peak(t, 0)
    return p if p is not None and p <= SSZ_STACK else None


def _series_root(typ, v) -> bytes:
    """hash_tree_root of a list or vector (ssz_impl.py:143-155), by the element's kind."""
    is_list = typ[0] == "list"
    elem = typ[1]
    n = len(v)
    if typ[0] == "vector" and n != typ[2]:
        raise ValueError("expected %d elements" % typ[2])
    if elem[0] in ("uint", "bool"):
        # packed (ssz_impl.py:110-119): the chunks of the serialization, zero-padded to 32 bytes
        data = bytes(v) if isinstance(v, (bytes, bytearray)) and elem == uint(1) else b"".join(
            serialize(elem, x) for x in v)
        data += b"\x00" * (-len(data) % 32)
        return merkle_root(data, chunk_depth(len(data) // 32), 0, n if is_list else None)
    if _program_fits(elem):
        # fixed-size composite elements: their roots, the tree and the length mix in one call
        size = item_size(elem)
        blob = b"".join(serialize(elem, x) for x in v)
        prog = compile_root(elem)
        out = ctypes.create_string_buffer(32)
        _native.check(_native.lib().bls381_ssz_list_root(n, blob or None, size, prog.ctypes.data_as(ctypes.c_void_p),
                                                         len(prog), 1 if is_list else 0, out))
        return out.raw
    if _ragged_fits(elem):
        # variable-size containers of basic lists: the same, the roots following each item's offsets
        return list_root_ragged(elem, [serialize(elem, x) for x in v], is_list)
    # the slow path: other variable-size elements (or ones too large for one lane), a call per element
    roots = [hash_tree_root(elem, x) for x in v]
    return merkle_root(roots, chunk_depth(n), 0, n if is_list else None)


def hash_tree_root(typ, value) -> bytes:
    """hash_tree_root of a Python value (ssz_impl.py:143-155).  A fixed-size type that fits one
    lane's 64-chunk stack is one root program; a list or vector goes by its element -- fixed-size
    composite: one bls381_ssz_list_root call; basic, and ``bytes``: one bls381_merkle_root over the
    zero-padded serialization; variable-size containers of basic lists: one
    bls381_ssz_ragged_list_root call; other variable-size elements: a root per element, then their
    tree (the slow path: one call per element) -- and a container with such fields combines its
    field roots through merkle_root, unless it has a ragged program of its own."""
    if _program_fits(typ):
        return hash_tree_root_batch(typ, [serialize(typ, value)])[0]
    if _ragged_fits(typ):
        return hash_tree_root_ragged_batch(typ, [serialize(typ, value)])[0][0]
    if typ[0] in ("list", "vector"):
        return _series_root(typ, value)
    if typ[0] == "bytes":      # a BytesN of more than 64 chunks
        return _series_root(Vector(uint(1), typ[1]), bytes(value))
    roots = [hash_tree_root(t, value[name]) for name, t in typ[1]]
    return merkle_root(roots, chunk_depth(len(roots)))


def signing_root(typ, value) -> bytes:
    """signing_root of a Python container value (ssz_impl.py:158-163): the last field left out."""
    if typ[0] != "container" or len(typ[1]) < 2:
        raise ValueError("signing_root needs a container with at least two fields")
    if _program_fits(typ, True):
        return signing_root_batch(typ, [serialize(typ, value)])[0]
    roots = [hash_tree_root(t, value[name]) for name, t in typ[1][:-1]]
    return merkle_root(roots, chunk_depth(len(roots)))
