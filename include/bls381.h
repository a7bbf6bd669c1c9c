/*
 * bls381.h -- C ABI of the MI355X (gfx950) BLS12-381 engine.
 *
 * Drop-in boundary for the reference's BLS path: every entry point below is
 * what `test_libs/pyspec/eth2spec/utils/bls.py` (reference) would bind through
 * ctypes in place of `from py_ecc import bls` (bls.py:1).  The Python mirror of
 * that module is consensus-specs_amd/bls381_amd/bls.py; the binding a
 * maintainer would add to the reference is shown in INTEGRATION.md.
 *
 * Conventions
 *   - Plain pointers and sizes only; the caller owns every buffer.
 *   - Pubkeys are 48-byte compressed G1, signatures 96-byte compressed G2
 *     (specs/bls_signature.md:36-64).  Messages are `msg_len` bytes (the spec's
 *     message_hash is Bytes32; py_ecc hashes any length, so 0..BLS381_MSG_MAX is accepted).
 *   - `dom8` is the 8-byte serialisation of the spec's uint64 `domain`
 *     (hash_to_G2, bls_signature.md:76-77).  The int -> bytes step is done by
 *     the caller so the byte order has one switch.
 *   - Return codes: >= 0 success (verdicts 1/0), < 0 error (BLS381_E*).
 *   - Host-pointer entry points copy to/from the device internally.  The
 *     `_device` variants take device pointers and a hipStream_t (as void*).
 *   - There is no CPU fallback: without a usable gfx950 device every call
 *     returns BLS381_ENODEV.
 *
 * Beside the BLS calls the header carries what produces and consumes their inputs
 * on the device: the pubkey registry, SSZ roots of fixed-size containers,
 * verify_merkle_branch and process_deposit, Merkle trees across items (roots and
 * proofs of utils/merkle_minimal.py's trees, list roots with mix_in_length, the
 * builder of Deposits with their proofs), and committee selection.
 */
#ifndef BLS381_H
#define BLS381_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BLS381_OK 0
#define BLS381_EINVAL_POINT (-1) /* an input point encoding is invalid (aggregate raises ValueError) */
#define BLS381_EARG (-2)         /* bad argument (NULL, length) */
#define BLS381_ENODEV (-3)       /* no HIP device / kernels not loadable */
#define BLS381_EHIP (-4)         /* HIP runtime error */
#define BLS381_MSG_MAX (1u << 20) /* message bytes per call (hash_to_G2 streams the message) */

/* Subgroup policy of the verify paths (DESIGN.md "Subgroup policy").
 *   PYECC (default): the checks py_ecc 1.7.0 makes, which the reference calls
 *     (bls.py:24-31): decoding and the on-curve test only.  Torsion of order
 *     prime to r in a pubkey leaves the verdict unchanged, and a signature with
 *     no G2 component whose Miller loop degenerates gives False -- both as py_ecc.
 *   STRICT: every pubkey and signature must also lie in G1 / G2, the spec's
 *     "valid G1/G2 point" (specs/bls_signature.md:135-136,143-144).
 * Aggregation never checks subgroups (py_ecc's aggregate_* do not). */
#define BLS381_POLICY_PYECC 0
#define BLS381_POLICY_STRICT 1

/* ---- runtime ----------------------------------------------------------- */
/* Number of visible HIP devices (0 if none). */
int bls381_device_count(void);
/* Select the device used by subsequent calls from this thread and create its
 * context (stream, workspace).  Idempotent. */
int bls381_init(int device);
/* Create the contexts of devices 0 .. n_devices-1 (SURVEY §8(b)'s bls381_init(n_devices);
 * a process driving several GPUs then selects one per thread with bls381_init). */
int bls381_init_devices(int n_devices);
void bls381_shutdown(void);
/* Last HIP error string of this thread (static storage). */
const char* bls381_last_error(void);
/* Process-wide subgroup policy (BLS381_POLICY_*), read when a call is queued.
 * Returns 0, or BLS381_EARG for an unknown policy.  Needs no device. */
int bls381_set_subgroup_policy(int policy);
int bls381_get_subgroup_policy(void);
/* Policy override for calls queued from the calling thread only (-1 clears it and the
 * thread follows the process-wide policy again).  The Python shim (bls.py) scopes each
 * verify with its module switch this way, so it neither rewrites the process-wide policy
 * that other front ends read nor races with other threads.  Returns 0 or BLS381_EARG. */
int bls381_set_thread_subgroup_policy(int policy);
/* The policy calls queued from this thread use (the override if set). */
int bls381_get_thread_subgroup_policy(void);
/* Kernel-time accounting (HIP events on the launch stream) for bench.py. */
int bls381_profile_enable(int on);
int bls381_profile_read(char* json_out, size_t cap);

/* ---- eth2spec.utils.bls drop-ins (reference bls.py:24-46) -------------- */

/* bls_verify (bls.py:24-26; bls_signature.md:131-137).  1 = valid, 0 = invalid
 * (including undecodable inputs, as py_ecc's except-clause returns False). */
int bls381_verify(const uint8_t pk[48], const uint8_t* msg, size_t msg_len,
                  const uint8_t sig[96], const uint8_t dom8[8]);

/* bls_verify_multiple (bls.py:29-31; bls_signature.md:139-146).  n pubkeys and
 * n messages of msg_len bytes each; pubkeys sharing a message are aggregated
 * first (py_ecc grouping) and one final exponentiation decides the call. */
int bls381_verify_multiple(size_t n, const uint8_t* pks, const uint8_t* msgs, size_t msg_len,
                           const uint8_t sig[96], const uint8_t dom8[8]);

/* bls_aggregate_pubkeys (bls.py:34-36): sum of n G1 points; n == 0 -> infinity.
 * Returns BLS381_EINVAL_POINT if any input does not decode. */
int bls381_aggregate_pubkeys(size_t n, const uint8_t* pks, uint8_t out[48]);

/* bls_aggregate_signatures (bls.py:39-41): sum of n G2 points. */
int bls381_aggregate_signatures(size_t n, const uint8_t* sigs, uint8_t out[96]);
/* SURVEY §8(b)'s names for the two aggregations (same behaviour). */
int bls381_aggregate_g1(size_t n, const uint8_t* pks, uint8_t out[48]);
int bls381_aggregate_g2(size_t n, const uint8_t* sigs, uint8_t out[96]);

/* bls_sign (bls.py:44-46): [sk] hash_to_G2(msg, domain); sk 32-byte big-endian. */
int bls381_sign(const uint8_t* msg, size_t msg_len, const uint8_t sk[32], const uint8_t dom8[8],
                uint8_t out[96]);

/* py_ecc bls.privtopub (test_generators/bls/main.py:114; helpers/keys.py:5). */
int bls381_privtopub(const uint8_t sk[32], uint8_t out[48]);

/* Batched sign / privtopub over n items (32-byte messages, 32-byte big-endian
 * secret keys, per-item dom8) -- used to build synthetic verify batches. */
int bls381_sign_batch(size_t n, const uint8_t* msgs32, const uint8_t* sks, const uint8_t* dom8s, uint8_t* out96);
int bls381_privtopub_batch(size_t n, const uint8_t* sks, uint8_t* out48);

/* hash_to_G2 (bls_signature.md:74-87; main.py:71,84): compressed (96 B) and
 * normalised affine x_re,x_im,y_re,y_im (4 x 48 B big-endian).  Either output may be NULL. */
int bls381_hash_to_g2(const uint8_t* msg, size_t msg_len, const uint8_t dom8[8],
                      uint8_t out_compressed[96], uint8_t out_affine[192]);

/* py_ecc's un-normalised projective triple for hash_to_G2 (main.py:56-72,
 * msg_hash_g2_uncompressed vectors): X,Y,Z each (re, im), 6 x 48 B big-endian.
 * n messages of 32 bytes with per-message dom8. */
int bls381_hash_to_g2_pyecc_projective(size_t n, const uint8_t* msgs32, const uint8_t* dom8s,
                                       uint8_t* out288);

/* ---- batched entry points (the throughput path) ------------------------ */

/* n independent bls_verify calls: verdicts_out[i] = 1/0. */
int bls381_verify_batch(size_t n, const uint8_t* pks, const uint8_t* msgs32, const uint8_t* sigs,
                        const uint8_t* dom8s, uint8_t* verdicts_out);

/* Device-resident variant: all pointers are device memory, stream = hipStream_t
 * (NULL = the HIP null stream, i.e. torch's default stream; work is queued, not synchronised).
 * `workspace` must hold bls381_verify_batch_workspace_size(n) bytes. */
size_t bls381_verify_batch_workspace_size(size_t n);
int bls381_verify_batch_device(size_t n, const uint8_t* d_pks, const uint8_t* d_msgs32,
                               const uint8_t* d_sigs, const uint8_t* d_dom8s, uint8_t* d_verdicts,
                               void* d_workspace, void* stream);

/* Opt-in randomized batch verification of n independent bls_verify items (the
 * north star's "batched Miller loops share a single final exponentiation"; SURVEY
 * §7 "Verdict semantics under batching").  Items go in sub-batches of `batch`
 * (even, 2 <= batch <= 32768; otherwise BLS381_EARG, and the workspace size is 0); a
 * sub-batch passes when
 *     prod_i e(H(m_i), [r_i] pk_i) * e(sum_i [r_i] sig_i, -g1) == 1,
 * r_i = k0 + mu k1 mod r, mu = -x^2, (k1, k0) = the first 8 bytes of
 * SHA-256(seed || i) as two 32-bit words (seed: 32 caller-chosen random bytes; 2^64
 * distinct weights, applied through the endomorphisms sigma / -psi^2: [r_i] pk_i as a joint
 * 32-bit multiplication, sum_i [r_i] sig_i as one bucket multi-scalar multiplication per
 * sub-batch), with one final exponentiation.  Items of a passing sub-batch are
 * valid (a wrong one slips through with probability <= 2^-63); every item of a failing sub-batch,
 * and every item whose signature is outside G2, is re-verified alone by the
 * default pipeline, so verdicts are the per-item ones.  The device form takes
 * device buffers, runs synchronously (the re-verification needs the sub-batch
 * results on the host) and, when stats != NULL, stores [items accepted in passing
 * sub-batches, items verified one by one, failed sub-batches]. */
int bls381_verify_batch_randomized(size_t n, const uint8_t* pks, const uint8_t* msgs32, const uint8_t* sigs,
                                   const uint8_t* dom8s, const uint8_t seed[32], size_t batch,
                                   uint8_t* verdicts_out);
size_t bls381_verify_batch_randomized_workspace_size(size_t n, size_t batch);
int bls381_verify_batch_randomized_device(size_t n, const uint8_t* d_pks, const uint8_t* d_msgs32,
                                          const uint8_t* d_sigs, const uint8_t* d_dom8s, const uint8_t seed[32],
                                          size_t batch, uint8_t* d_verdicts, void* d_workspace, void* stream,
                                          uint64_t* stats);

/* Committee aggregation (config C3/C4): n_groups groups, group g = pubkeys
 * [offsets[g], offsets[g+1]).  out48 receives n_groups compressed sums; status[g]
 * is 0, or BLS381_EINVAL_POINT when a member does not decode. */
int bls381_aggregate_pubkeys_batch(size_t n_groups, const uint32_t* offsets, const uint8_t* pks,
                                   uint8_t* out48, int32_t* status);
size_t bls381_aggregate_pubkeys_batch_workspace_size(size_t n_groups, size_t n_pks);
/* h_offsets is a HOST array (n_groups + 1 entries): the grouping plan is built on the host. */
int bls381_aggregate_pubkeys_batch_device(size_t n_groups, const uint32_t* h_offsets, size_t n_pks,
                                          const uint8_t* d_pks, uint8_t* d_out48, int32_t* d_status,
                                          void* d_workspace, void* stream);

/* n_calls independent bls_verify_multiple calls: call c
 * owns pubkeys/messages [call_off[c], call_off[c+1]) (host offsets, n_calls+1
 * entries), signature sigs[c] (96 B) and dom8s[c] (8 B).  verdicts[c] = 1/0. */
int bls381_verify_multiple_batch(size_t n_calls, const uint32_t* call_off, const uint8_t* pks,
                                 const uint8_t* msgs, size_t msg_len, const uint8_t* sigs, const uint8_t* dom8s,
                                 uint8_t* verdicts);

/* Device-resident form (C3: the committee aggregates never leave HBM).  Pubkeys
 * (d_pks, 48 B each, numbered like the messages), signatures (d_sigs, 96 B per
 * call) and domains (d_dom8s) are device memory; the call offsets and the
 * messages stay on the HOST (h_call_off, h_msgs): they decide the per-message
 * grouping plan, and the messages are copied with it.  d_verdicts[c] = 1/0.  Work
 * is queued on `stream` (hipStream_t; NULL = the null stream), not synchronised.
 * The workspace must hold bls381_verify_multiple_batch_workspace_size bytes. */
size_t bls381_verify_multiple_batch_workspace_size(size_t n_calls, size_t n_pks, size_t msg_len);
int bls381_verify_multiple_batch_device(size_t n_calls, const uint32_t* h_call_off, const uint8_t* h_msgs,
                                        size_t msg_len, const uint8_t* d_pks, const uint8_t* d_sigs,
                                        const uint8_t* d_dom8s, uint8_t* d_verdicts, void* d_workspace,
                                        void* stream);

/* Batched validate_indexed_attestation (reference 0_beacon-chain.md:1023-1026):
 *   bls_verify_multiple(pubkeys=[bls_aggregate_pubkeys(group) for group in call c],
 *                       message_hashes=[one message per group], signature, domain)
 * in one call, with the aggregation fused in: call c owns groups
 * [h_call_group_off[c], h_call_group_off[c+1]); group g owns the member keys
 * d_pks[h_group_key_off[g] .. h_group_key_off[g+1]) (48 B each, device memory, in
 * group order) and message h_group_msgs[g] (msg_len bytes, host).  The members' sum
 * runs beside hash_to_G2 instead of before it.  An empty group is the infinite
 * aggregate (its pairing is 1); groups of one call with equal messages are merged, as
 * py_ecc's verify_multiple does.  Divergence: an undecodable member key makes the
 * verdict 0 where bls_aggregate_pubkeys would raise.  Queued on `stream`, not
 * synchronised; the workspace must hold bls381_verify_multiple_grouped_workspace_size. */
size_t bls381_verify_multiple_grouped_workspace_size(size_t n_calls, size_t n_groups, size_t n_pks,
                                                     size_t msg_len);
int bls381_verify_multiple_grouped_device(size_t n_calls, const uint32_t* h_call_group_off, size_t n_groups,
                                          const uint32_t* h_group_key_off, const uint8_t* h_group_msgs,
                                          size_t msg_len, const uint8_t* d_pks, const uint8_t* d_sigs,
                                          const uint8_t* d_dom8s, uint8_t* d_verdicts, void* d_workspace,
                                          void* stream);

/* ---- multi-GPU partial products --------------------------- */
/* Miller-loop product of one shard of a bls_verify_multiple call: pairs
 * (hash_to_G2(msg_g), group_pubkey_g) for the messages in this shard, plus
 * (sig, -g1) when include_sig != 0.  out576 = Fp12 in the engine's tower
 * (a0..b2, each re||im, 48-byte big-endian).  Returns 0, or 1 when an input
 * fails to decode / fails a subgroup check (the call's verdict is then False). */
int bls381_miller_partial(size_t n, const uint8_t* pks, const uint8_t* msgs, size_t msg_len,
                          const uint8_t sig[96], int include_sig, const uint8_t dom8[8],
                          uint8_t out576[576]);
/* Multiply k partial products and run one final exponentiation: 1 / 0. */
int bls381_final_verify(size_t k, const uint8_t* parts576);

/* ---- native multi-GPU over RCCL: one process per GPU -------- */
/* A communicator lives inside the library (RCCL opened with dlopen on first
 * use).  Rank 0 makes a 128-byte id, the launcher hands it to every rank (any
 * channel: bls381_amd/comm.py uses TCP), each rank calls bls381_comm_init on the
 * device it selected with bls381_init.  No PyTorch anywhere. */
int bls381_comm_unique_id(uint8_t out[128]);
int bls381_comm_init(int nranks, int rank, const uint8_t uid[128]);
/* Path of the RCCL shared object the library uses (an RCCL the process already loaded,
 * e.g. PyTorch's, is preferred over a fresh dlopen; needs no device).  0, or ENODEV. */
int bls381_comm_rccl_path(char* out, size_t cap);
/* One process plays all nranks ranks on its own GPU: the same partition and
 * rank-0 combination, the all-gather a device copy (RCCL refuses two ranks on
 * one GPU; this is how a one-GPU box runs the N-rank protocol). */
int bls381_comm_init_virtual(int nranks);
int bls381_comm_size(void);   /* 0 without a communicator */
int bls381_comm_rank(void);   /* -1 without a communicator */
void bls381_comm_destroy(void);
/* Collective bls_verify_multiple (every rank passes the same call): distinct
 * message k goes to rank k mod nranks (its pubkey group never straddles ranks),
 * rank 0 adds (sig, -g1); each rank's Miller product (576 B, zero if a member is
 * invalid) is all-gathered over RCCL and rank 0 multiplies them and runs the one
 * final exponentiation of the call (py_ecc's single-FE semantics,
 * 1_custody-game.md:409); the verdict is broadcast.  Returns 1 / 0 on every rank. */
int bls381_verify_multiple_sharded(size_t n, const uint8_t* pks, const uint8_t* msgs, size_t msg_len,
                                   const uint8_t sig[96], const uint8_t dom8[8]);
/* Collective bls_aggregate_pubkeys: contiguous pubkey ranges per rank, compressed
 * partials all-gathered and summed on rank 0, broadcast.  Returns 0 or
 * BLS381_EINVAL_POINT (any rank's invalid encoding) on every rank. */
int bls381_aggregate_pubkeys_sharded(size_t n, const uint8_t* pks, uint8_t out[48]);
/* Device-resident form: this rank's n_local keys (its contiguous range of the call, in rank
 * order; a virtual communicator takes the whole call) are already in HBM at d_pks; every rank
 * receives the aggregate in d_out48 and the status (0 or BLS381_EINVAL_POINT) in d_status[0],
 * queued on `stream` with no host copy and no synchronisation.  Replaces the host-buffer form's
 * PCIe copies for callers whose keys are device-resident (bls.py:34-36 aggregate_pubkeys,
 * SURVEY.md §8e).  Returns 0 or a launch / RCCL error code. */
size_t bls381_aggregate_pubkeys_sharded_device_workspace_size(size_t n_local);
int bls381_aggregate_pubkeys_sharded_device(size_t n_local, const uint8_t* d_pks, uint8_t* d_out48,
                                            int32_t* d_status, void* d_workspace, void* stream);
/* Independent verify_multiple calls, contiguous call ranges per rank (a call's
 * final exponentiation is never split); every rank receives all verdicts. */
int bls381_verify_multiple_batch_sharded(size_t n_calls, const uint32_t* call_off, const uint8_t* pks,
                                         const uint8_t* msgs, size_t msg_len, const uint8_t* sigs,
                                         const uint8_t* dom8s, uint8_t* verdicts);

/* ---- device-resident pubkey registry ---------------- */
/* Decoded validator pubkeys kept in HBM, so committee aggregation reads each
 * member's point instead of decompressing it (the per-key Fp square root that
 * dominates bls_aggregate_pubkeys).  The reference indexes pubkeys through
 * state.validator_registry (specs/core/0_beacon-chain.md:1025-1026, the
 * get_attesting_indices -> bls_aggregate_pubkeys call of
 * validate_indexed_attestation); aggregation over the registry returns the same
 * bytes as bls_aggregate_pubkeys over the members' encodings (bls.py:34-36).
 * Entries are appended in order: entry e is the e-th key ever added (the
 * validator index when keys are added in registry order).  One registry belongs
 * to the device current at creation. */
typedef struct bls381_registry bls381_registry;
int bls381_registry_create(size_t capacity, bls381_registry** out);
void bls381_registry_destroy(bls381_registry* reg);
size_t bls381_registry_size(const bls381_registry* reg);
/* Append n keys as entries [size, size+n).  entry_out[i] (may be NULL) is the
 * entry that now holds key i's bytes (its own, or an earlier duplicate's), or
 * -1 when key i does not decode.  Returns the number of keys that do not decode. */
int bls381_registry_add(bls381_registry* reg, size_t n, const uint8_t* pks48, int32_t* entry_out);
/* Content-addressed lookup: entry_out[i] = entry holding key i's bytes, or -1.
 * Returns the number of hits. */
int bls381_registry_lookup(bls381_registry* reg, size_t n, const uint8_t* pks48, int32_t* entry_out);
/* Group g = entries indices[offsets[g] .. offsets[g+1]); status as for
 * bls381_aggregate_pubkeys_batch (an undecodable or out-of-range entry makes
 * its group BLS381_EINVAL_POINT). */
int bls381_registry_aggregate_indices(bls381_registry* reg, size_t n_groups, const uint32_t* offsets,
                                      const uint32_t* indices, uint8_t* out48, int32_t* status);
/* Same contract as bls381_aggregate_pubkeys_batch: members found in the
 * registry are read from it, the others are decoded from their bytes. */
int bls381_registry_aggregate_pubkeys_batch(bls381_registry* reg, size_t n_groups, const uint32_t* offsets,
                                            const uint8_t* pks, uint8_t* out48, int32_t* status);
size_t bls381_registry_aggregate_workspace_size(size_t n_groups, size_t n_idx);
/* Device-pointer form of bls381_registry_aggregate_indices (h_offsets on the host). */
int bls381_registry_aggregate_indices_device(bls381_registry* reg, size_t n_groups, const uint32_t* h_offsets,
                                             size_t n_idx, const uint32_t* d_indices, uint8_t* d_out48,
                                             int32_t* d_status, void* d_workspace, void* stream);

/* bls381_verify_multiple_grouped_device with the member keys given as registry entries
 * (d_entries: one uint32 entry per member, in group order; the reference's
 * state.validator_registry[i].pubkey, 0_beacon-chain.md:1025-1026): the committee sums
 * add decoded registry points instead of decoding every member.  An entry past the
 * registry's end, or one holding an undecodable key, makes the verdict 0.  Workspace:
 * bls381_verify_multiple_grouped_workspace_size. */
int bls381_registry_verify_multiple_grouped_device(bls381_registry* reg, size_t n_calls,
                                                   const uint32_t* h_call_group_off, size_t n_groups,
                                                   const uint32_t* h_group_key_off, const uint8_t* h_group_msgs,
                                                   size_t msg_len, const uint32_t* d_entries, const uint8_t* d_sigs,
                                                   const uint8_t* d_dom8s, uint8_t* d_verdicts, void* d_workspace,
                                                   void* stream);

/* ---- SSZ roots: the message_hash producer ---------- */
/* hash_tree_root / signing_root of n serialized fixed-size SSZ items
 * (test_libs/pyspec/eth2spec/utils/ssz/ssz_impl.py:143-163, merkle_minimal.py
 * merkleize_chunks).  `prog` is the item type compiled by bls381_amd/ssz.py:
 * words {1, off, len} push bytes [off, off+len) zero-padded to a 32-byte chunk
 * (len <= 32); {2, k} merkleizes the top k chunks (zero-padded to a power of
 * two) into one.  The program must leave exactly one chunk, read only inside
 * the item, and fit 512 words / 64 chunks, else BLS381_EARG.  roots32 receives
 * n x 32 bytes. */
int bls381_ssz_root_batch(size_t n, const uint8_t* items, size_t item_size, const uint32_t* prog,
                          uint32_t prog_len, uint8_t* roots32);
size_t bls381_ssz_root_workspace_size(void);
/* Device form: item i at d_items + i * stride (stride >= item_size); h_prog on the host. */
int bls381_ssz_root_batch_device(size_t n, const uint8_t* d_items, size_t stride, size_t item_size,
                                 const uint32_t* h_prog, uint32_t prog_len, uint8_t* d_roots32,
                                 void* d_workspace, void* stream);
/* process_deposit's proof-of-possession check over n serialized DepositData
 * (184 B each: pubkey, withdrawal_credentials, amount, signature;
 * 0_beacon-chain.md:394-403): verdicts[i] = bls_verify(pubkey,
 * signing_root(deposit.data), signature, domain) (0_beacon-chain.md:1755-1758),
 * the signing roots computed on the device and fed straight to the verify
 * pipeline. */
int bls381_verify_deposits(size_t n, const uint8_t* deposit_data, const uint8_t* dom8s, uint8_t* verdicts);
size_t bls381_verify_deposits_workspace_size(size_t n);
int bls381_verify_deposits_device(size_t n, const uint8_t* d_deposit_data, const uint8_t* d_dom8s,
                                  uint8_t* d_verdicts, void* d_workspace, void* stream);

/* ---- Merkle branches and process_deposit over the registry -------------- */
/* verify_merkle_branch (0_beacon-chain.md:846-857; also the custody game and
 * light_client/sync_protocol.md) for n items, one lane each:
 *   ok_out[i] = verify_merkle_branch(leaves32[i], proofs[i*depth .. ), depth, indices[i], root_i)
 * with 32-byte siblings, proofs packed (depth * 32 bytes per item), bit k of the 64-bit
 * indices[i] choosing the side of sibling k, and root_i = roots32 + i * root_stride;
 * root_stride is 0 (one root for all items) or 32.  depth == 0 compares the leaf with the
 * root (proofs may then be NULL).  depth > 64, another root_stride, or a NULL argument with
 * n > 0 return BLS381_EARG.  The device form is queued on `stream` (not synchronised) and
 * needs no workspace; d_indices must be 8-byte aligned. */
int bls381_merkle_branch_batch(size_t n, const uint8_t* leaves32, const uint8_t* proofs, uint32_t depth,
                               const uint64_t* indices, const uint8_t* roots32, size_t root_stride,
                               uint8_t* ok_out);
int bls381_merkle_branch_batch_device(size_t n, const uint8_t* d_leaves32, const uint8_t* d_proofs, uint32_t depth,
                                      const uint64_t* d_indices, const uint8_t* d_roots32, size_t root_stride,
                                      uint8_t* d_ok, void* stream);

/* process_deposit (0_beacon-chain.md:1732-1775) for n serialized Deposits (:457-461:
 * 32 x 32 B of proof, then the 184 B DepositData), with the semantics of calling it on
 * deposits 0 .. n-1 in order: state.deposit_index starts at first_index, and the validator
 * pubkeys are the registry's entries.
 *   *first_bad_proof  the first i whose branch does not lead from hash_tree_root(deposit.data)
 *       to deposit_root under index first_index + i (the spec's assert), or -1.  When it is
 *       >= 0 the registry is left untouched whatever `commit` says, and the call returns 0.
 *   outcome[i]        BLS381_DEPOSIT_*; never depends on the proofs, always filled.  A deposit
 *       for a key that is registered -- before the call, or by an earlier deposit of this
 *       batch whose proof of possession held -- is a TOPUP and its signature is not checked; a
 *       new key with a valid proof of possession is NEW; with an invalid one, SKIPPED.
 *   validator_index[i]  the entry that holds the key: for a key NEW in this batch,
 *       size_before + (number of NEW among deposits < i); -1 for a SKIPPED deposit.
 * Returns the number of NEW deposits, or an error code.  With commit != 0 (and every proof
 * good) the NEW keys are appended in deposit order, decoded and entered in the table as by
 * bls381_registry_add; bls381_registry_size and later lookups, aggregations and grouped
 * verifies see them when the call returns.  If they do not fit the capacity the call returns
 * BLS381_EARG and the registry is unchanged.  With commit == 0 nothing changes.  Entries
 * equal validator indices as long as every earlier addition was unique; this call keeps that.
 * The subgroup policy of the proof-of-possession check is the calling thread's.
 * Divergence: membership is by key bytes in the registry's table, which omits undecodable
 * keys.  A registry that was fed an undecodable key through bls381_registry_add treats a
 * deposit for it as new, and the deposit is then SKIPPED (its proof of possession cannot
 * hold); a registry grown only by this call cannot hold such a key.
 * deposit_root and dom8 are host memory in both forms.  The device form takes device
 * buffers (d_workspace of bls381_registry_process_deposits_workspace_size(n) bytes) and runs
 * synchronously -- the host needs the count and the proof flag before the registry's size
 * moves -- as bls381_verify_batch_randomized_device does. */
#define BLS381_DEPOSIT_BYTES 1208
#define BLS381_DEPOSIT_SKIPPED 0 /* new key, proof of possession invalid: the spec's early return */
#define BLS381_DEPOSIT_NEW 1     /* validator appended (or would be, commit == 0) */
#define BLS381_DEPOSIT_TOPUP 2   /* key already a validator: balance increase, signature not checked */
int bls381_registry_process_deposits(bls381_registry* reg, size_t n, const uint8_t* deposits, uint64_t first_index,
                                     const uint8_t deposit_root[32], const uint8_t dom8[8], int commit,
                                     uint8_t* outcome, int32_t* validator_index, int64_t* first_bad_proof);
size_t bls381_registry_process_deposits_workspace_size(size_t n);
int bls381_registry_process_deposits_device(bls381_registry* reg, size_t n, const uint8_t* d_deposits,
                                            uint64_t first_index, const uint8_t deposit_root[32],
                                            const uint8_t dom8[8], int commit, uint8_t* d_outcome,
                                            int32_t* d_validator_index, int64_t* first_bad_proof, void* d_workspace,
                                            void* stream);

/* ---- Merkle trees across items: list roots, deposit trees and proofs ----- */
/* tree(leaves32[0..n), first, depth) is the tree with 2^depth leaves of which leaves
 * first .. first+n-1 are given (32 bytes each) and every other one is the zero chunk; H is
 * SHA-256, Z[0] = 32 zero bytes, Z[h+1] = H(Z[h] || Z[h]).  Node (h, j) covers leaves
 * [j 2^h, (j+1) 2^h) and is Z[h] when that span misses the window.  This is the reference's
 * utils/merkle_minimal.py: get_merkle_root / get_merkle_proof are first = 0, depth = 32 (a
 * window with first > 0 is their tree over [ZERO] * first + leaves), merkleize_chunks is first = 0,
 * depth = ceil(log2 n).  Extension: n == 0 is valid and gives Z[depth], the deposit contract's
 * empty root, where the reference's get_merkle_root([]) raises.
 *   root    node (depth, 0); with mix_length != 0 it is then mixed with `length`:
 *           mix_in_length(root, length) = H(root || length as 32 bytes little-endian)
 *           (ssz_impl.py:122-124).
 *   proofs  for each of the n_idx leaf indices i, sibling h = node (h, (i >> h) ^ 1) for
 *           h = 0 .. depth-1, 32 bytes each, at proofs + k * proof_stride (proof_stride >=
 *           32 * depth; bytes of a row past the proof are left alone, so proofs can land in
 *           the first 1,024 bytes of 1,208-byte Deposit records).  An index outside the window
 *           gets the proof of a zero leaf; indices are meant to be below 2^depth.  With
 *           depth == 0 nothing is written.  The root is not mixed.
 * BLS381_EARG: depth > 64, first + n overflowing or above 2^depth, n or n_idx above 2^31 - 1,
 * a proof_stride below 32 * depth, or a NULL argument that is needed (leaves with n > 0;
 * indices and proofs with n_idx > 0; the root and, in the device forms, the workspace always).
 * The device forms are queued on `stream`, not synchronised; d_leaves32, d_proofs and proof_stride
 * are 4-byte aligned and d_indices 8-byte aligned (else BLS381_EARG); the workspace holds
 * bls381_merkle_root_workspace_size / bls381_merkle_proofs_workspace_size bytes (0 for arguments
 * the call rejects). */
size_t bls381_merkle_root_workspace_size(size_t n, uint64_t first, uint32_t depth);
int bls381_merkle_root(size_t n, const uint8_t* leaves32, uint64_t first, uint32_t depth, int mix_length,
                       uint64_t length, uint8_t root[32]);
int bls381_merkle_root_device(size_t n, const uint8_t* d_leaves32, uint64_t first, uint32_t depth, int mix_length,
                              uint64_t length, uint8_t* d_root32, void* d_workspace, void* stream);
size_t bls381_merkle_proofs_workspace_size(size_t n, uint64_t first, uint32_t depth);
int bls381_merkle_proofs(size_t n, const uint8_t* leaves32, uint64_t first, uint32_t depth, size_t n_idx,
                         const uint64_t* indices, uint8_t* proofs, size_t proof_stride, uint8_t root[32]);
int bls381_merkle_proofs_device(size_t n, const uint8_t* d_leaves32, uint64_t first, uint32_t depth, size_t n_idx,
                                const uint64_t* d_indices, uint8_t* d_proofs, size_t proof_stride, uint8_t* d_root32,
                                void* d_workspace, void* stream);

/* hash_tree_root of a List or Vector of n fixed-size composite elements (ssz_impl.py:143-155):
 * the n items through a root program (as bls381_ssz_root_batch), then the tree of depth
 * ceil(log2 n) over their roots, then mix_in_length(n) when mix_length != 0 (a List; a Vector
 * has none).  n == 0 gives the zero chunk, mixed with 0 for a list.  BLS381_EARG as for
 * bls381_ssz_root_batch, and for n above 2^31 - 1. */
size_t bls381_ssz_list_root_workspace_size(size_t n);
int bls381_ssz_list_root(size_t n, const uint8_t* items, size_t item_size, const uint32_t* prog, uint32_t prog_len,
                         int mix_length, uint8_t root[32]);
int bls381_ssz_list_root_device(size_t n, const uint8_t* d_items, size_t stride, size_t item_size,
                                const uint32_t* h_prog, uint32_t prog_len, int mix_length, uint8_t* d_root32,
                                void* d_workspace, void* stream);

/* Roots of n variable-size items in one call: attestations, pending and
 * indexed attestations, attester slashings.  Item i is bytes [starts[i], starts[i+1]) of `items`:
 * the SSZ serialization of a container whose variable-size fields are lists of basic elements
 * (`bytes` included) or such containers again (ssz_impl.py:72-103: fixed parts with a 4-byte
 * little-endian offset in place of each variable field, then the variable parts).  `prog` is the
 * type compiled by bls381_amd/ssz.py: {3, fixed} opens it (the fixed part's bytes); {1, off, len}
 * and {2, k} are as in bls381_ssz_root_batch, off inside the fixed part of the current scope;
 * {4, pos, next, esz} pushes the root of the basic list whose offset word is at `pos` and which
 * ends at the offset at `next` (0xffffffff: with the scope), elements of esz bytes, its length
 * mixed in; {5, pos, next, fixed} enters the container at that field, {6} leaves it.
 * Items are untrusted.  One is well formed when in every scope: the scope is at least as long as
 * its fixed part; the first offset equals the fixed part's size; offsets do not decrease; the last
 * is at most the scope's length; a field's length is a multiple of its element size.  A malformed
 * item gets status[i] = 1 and an all-zero root (a well-formed one status 0), no byte outside its
 * range is read for it, and the other items are unaffected.
 *   roots        n x 32 bytes and n status bytes.
 *   list_root    hash_tree_root of the list of the n items: the tree of depth ceil(log2 n) over
 *                their roots, mix_in_length(n) when mix_length != 0; n == 0 gives the empty list's
 *                root.  *n_bad (may be NULL in the host form) receives the count of malformed
 *                items; the host form then returns BLS381_EARG and leaves root[] alone, the device
 *                form leaves the count in the device word d_n_bad for the caller to look at (the
 *                root is then that of the list with zero chunks for those items).
 * Device forms take the offsets in device memory and items_bytes, the size of the d_items buffer:
 * a range that decreases, ends past items_bytes or spans 2^32 bytes or more is a malformed item.
 * They queue a number of launches that depends on n alone, never synchronise and read nothing back.
 * BLS381_EARG, found on the host: a program that is not well formed (512 words, 64 chunks of stack
 * with 28 for the longest field a 32-bit offset admits, scopes 4 deep, chunk reads and offset
 * words inside the fixed part); host-form starts that decrease, or an item of 2^32 bytes or more;
 * n above 2^31 - 1; a NULL pointer that is needed; d_roots32, d_root32 and d_n_bad not 4-byte or
 * d_starts not 8-byte aligned. */
size_t bls381_ssz_ragged_roots_workspace_size(size_t n);
int bls381_ssz_ragged_roots(size_t n, const uint8_t* items, const uint64_t* starts, const uint32_t* prog,
                            uint32_t prog_len, uint8_t* roots32, uint8_t* status);
int bls381_ssz_ragged_roots_device(size_t n, const uint8_t* d_items, size_t items_bytes, const uint64_t* d_starts,
                                   const uint32_t* h_prog, uint32_t prog_len, uint8_t* d_roots32, uint8_t* d_status,
                                   uint32_t* d_n_bad, void* d_workspace, void* stream);
size_t bls381_ssz_ragged_list_root_workspace_size(size_t n);
int bls381_ssz_ragged_list_root(size_t n, const uint8_t* items, const uint64_t* starts, const uint32_t* prog,
                                uint32_t prog_len, int mix_length, uint8_t root[32], uint32_t* n_bad);
int bls381_ssz_ragged_list_root_device(size_t n, const uint8_t* d_items, size_t items_bytes, const uint64_t* d_starts,
                                       const uint32_t* h_prog, uint32_t prog_len, int mix_length, uint8_t* d_root32,
                                       uint32_t* d_n_bad, void* d_workspace, void* stream);

/* n serialized DepositData (184 B each) -> n serialized Deposits (1,208 B: the 32-sibling proof,
 * then the data) under one deposit root: leaf first_index + i is hash_tree_root(data i), every
 * other leaf of the depth-32 tree is zero (the reference's test/helpers/deposits.py build, the
 * input of bls381_registry_process_deposits with the same first_index and root).
 * BLS381_EARG: first_index + n above 2^32, n above 2^31 - 1, a NULL argument that is needed;
 * d_deposits is 4-byte aligned. */
size_t bls381_deposits_build_workspace_size(size_t n);
int bls381_deposits_build(size_t n, const uint8_t* deposit_data, uint64_t first_index, uint8_t* deposits,
                          uint8_t deposit_root[32]);
int bls381_deposits_build_device(size_t n, const uint8_t* d_deposit_data, uint64_t first_index, uint8_t* d_deposits,
                                 uint8_t* d_deposit_root32, void* d_workspace, void* stream);

/* ---- the deposit tree kept on the device: append, roots and proofs at any count ---- */
/* A tree of 2^depth leaves (depth <= 32, the deposit contract's 32) that lives in device memory,
 * grows by appends and answers for every count k up to the current one what the contract
 * answers at that count: root(k) = get_deposit_root() after k deposits = the reference's
 * get_merkle_root(leaves[:k]), and proofs under it (get_merkle_proof).  A block's deposits carry
 * proofs against state.latest_eth1_data.deposit_root (0_beacon-chain.md:1630, :1742), the root
 * at the voted count: not the tree of the block's batch, which is what bls381_deposits_build
 * makes, and not the newest root.  Queries for a count are not disturbed by later appends: they
 * read only nodes that were complete at that count.
 * The tree belongs to the device current at creation (calls with another device current return
 * BLS381_EARG) and holds about 64 bytes per leaf of capacity.  One thread and one stream at a
 * time use a tree, or the caller orders them: the host-pointer forms run on the engine's own
 * stream and return synchronised, the device forms are queued on `stream`, not synchronised.
 * The count is kept on the host and moves when an append is queued.
 *   create   the capacity is fixed.  BLS381_EARG for depth > 32, capacity == 0 or capacity >
 *            2^depth - 1 (the contract's MAX_DEPOSIT_COUNT assert; depth 0 has no valid capacity).
 *   append   leaves count .. count+n-1 become the n given 32-byte values; append_data takes n
 *            serialized DepositData (184 B each) and appends leaf = hash_tree_root(data), hashed
 *            straight into the tree.  n == 0 is BLS381_OK and runs nothing; count + n > capacity
 *            is BLS381_EARG and leaves the tree unchanged.
 *   roots    roots32[q] = the root of the depth-`depth` tree over the first counts[q] leaves with
 *            zeros behind them; counts[q] == 0 gives Z[depth].  counts is host memory in both
 *            forms.  Any counts[q] above the count is BLS381_EARG.
 *   proofs   siblings 0 .. depth-1 of each index in the tree at count k, and that tree's root,
 *            with the proof rows of bls381_merkle_proofs: proof_stride >= 32 * depth, bytes of a
 *            row past the proof left alone; d_proofs and proof_stride 4-byte, d_indices 8-byte
 *            aligned in the device form.  An index >= k gets the proof of a zero leaf.  k above
 *            the count is BLS381_EARG.
 *   deposits n serialized Deposits (1,208 B) for leaves first_index .. first_index+n-1: the proof
 *            under the root at count k, then deposit_data[i] (184 B each) copied behind it; the
 *            input of bls381_registry_process_deposits with the same first_index and
 *            roots([k]).  Needs depth == 32 and first_index + n <= k <= count, else BLS381_EARG.
 *            The data is NOT re-hashed against the stored leaves: handing in other data than was
 *            appended gives deposits whose proofs fail.
 * m, n and n_idx are at most 2^31 - 1; a NULL argument that is needed is BLS381_EARG (the tree
 * always; data and outputs when the count of items is not 0; the root of `proofs` and the
 * workspaces of the device forms always).  In the device forms d_leaves32, d_roots32 and
 * d_deposits are 4-byte aligned as well, else BLS381_EARG.  Workspaces hold bls381_deposit_tree_*_workspace_size
 * bytes (0 for arguments the call rejects) and belong to the call: a tree has no scratch of its
 * own that a second queued call could overwrite. */
typedef struct bls381_deposit_tree bls381_deposit_tree;
int bls381_deposit_tree_create(size_t capacity, uint32_t depth, bls381_deposit_tree** out);
void bls381_deposit_tree_destroy(bls381_deposit_tree* tree);
size_t bls381_deposit_tree_count(const bls381_deposit_tree* tree);
size_t bls381_deposit_tree_capacity(const bls381_deposit_tree* tree);
int bls381_deposit_tree_append(bls381_deposit_tree* tree, size_t n, const uint8_t* leaves32);
int bls381_deposit_tree_append_device(bls381_deposit_tree* tree, size_t n, const uint8_t* d_leaves32, void* stream);
size_t bls381_deposit_tree_append_data_workspace_size(size_t n);
int bls381_deposit_tree_append_data(bls381_deposit_tree* tree, size_t n, const uint8_t* deposit_data);
int bls381_deposit_tree_append_data_device(bls381_deposit_tree* tree, size_t n, const uint8_t* d_deposit_data,
                                           void* d_workspace, void* stream);
int bls381_deposit_tree_roots(bls381_deposit_tree* tree, size_t m, const uint64_t* counts, uint8_t* roots32);
int bls381_deposit_tree_roots_device(bls381_deposit_tree* tree, size_t m, const uint64_t* h_counts, uint8_t* d_roots32,
                                     void* stream);
size_t bls381_deposit_tree_proofs_workspace_size(uint32_t depth);
int bls381_deposit_tree_proofs(bls381_deposit_tree* tree, uint64_t k, size_t n_idx, const uint64_t* indices,
                               uint8_t* proofs, size_t proof_stride, uint8_t root[32]);
int bls381_deposit_tree_proofs_device(bls381_deposit_tree* tree, uint64_t k, size_t n_idx, const uint64_t* d_indices,
                                      uint8_t* d_proofs, size_t proof_stride, uint8_t* d_root32, void* d_workspace,
                                      void* stream);
size_t bls381_deposit_tree_deposits_workspace_size(size_t n);
int bls381_deposit_tree_deposits(bls381_deposit_tree* tree, uint64_t k, uint64_t first_index, size_t n,
                                 const uint8_t* deposit_data, uint8_t* deposits);
int bls381_deposit_tree_deposits_device(bls381_deposit_tree* tree, uint64_t k, uint64_t first_index, size_t n,
                                        const uint8_t* d_deposit_data, uint8_t* d_deposits, void* d_workspace,
                                        void* stream);

/* ---- SSZ list trees kept on the device: update items, re-root by dirty paths ---- */
/* A list of count <= capacity items of item_size bytes, packed, that lives in device memory with
 * the Merkle tree over its chunks, takes in-place updates as well as appends, and re-hashes only
 * the tiles on the paths of what changed: state.validator_registry,
 * state.balances and the root vectors held across slots.  The mode is fixed at creation.
 *   composite (prog != NULL): chunk i is the root program over item i, as in bls381_ssz_root_batch,
 *            with its checks (a well-formed program of at most 512 words and 64 chunks that reads
 *            inside the item).  List[Validator], any list or vector of fixed-size containers.
 *   packed   (prog == NULL, prog_len == 0): item_size is 1, 2, 4, 8, 16 or 32 and chunk j is bytes
 *            [32 j, 32 j + 32) of the packed items, zero behind the last item.  List[uint64],
 *            Vector[Bytes32, N].
 * With `chunks` the number of chunks at the current count and d = ceil(log2 chunks) (0 for
 * chunks <= 1):
 *   root     node (d, 0) of the tree over the chunks with zero chunks behind them, and with
 *            mix_length != 0 mix_in_length(root, count): after every sequence of operations what
 *            bls381_ssz_list_root (composite) or bls381_merkle_root(n = chunks, first = 0, depth =
 *            d, mix_length, length = count) (packed) gives over the items as they stand.  count ==
 *            0 gives the zero chunk, mixed with 0 when asked.  d moves as the list grows.
 *   append   items count .. count+n-1.  count + n > capacity is BLS381_EARG and nothing changes;
 *            n == 0 is BLS381_OK and runs nothing.
 *   update   bytes [off, off+len) of item indices[t] become values[t len .. (t+1) len): off = 0,
 *            len = item_size replaces items; off = 113, len = 8 on Validator records sets
 *            effective_balance.  off + len > item_size is BLS381_EARG; len == 0 or n_upd == 0 is
 *            BLS381_OK and runs nothing.  Host-pointer form: an index at or above the count is
 *            BLS381_EARG and nothing changes; repeated indices are applied in order (the last
 *            wins).  Device form: the host does not see the indices; an index at or above the
 *            count is skipped; repeated indices with byte-equal values are fine, with different
 *            values each byte ends up holding one of the given values.  In every case the tree is
 *            afterwards the tree of what the store holds: leaves are re-hashed from the store.
 *   proofs   siblings 0 .. d-1 of each chunk index at the current count and the unmixed root,
 *            with the proof rows of bls381_merkle_proofs: proof_stride >= 32 d, bytes of a row
 *            past the proof left alone; a chunk index at or above `chunks` (and below 2^d) gets
 *            the proof of a zero chunk; with d == 0 nothing is written.  They verify under
 *            bls381_merkle_branch_batch(depth = d).  There are no queries at earlier counts
 *            (in-place updates rule them out: that is the deposit tree's job).
 *   read     copies items [first, first+n) to the host; first + n above the count is BLS381_EARG.
 *   items_device  the device address of item 0 (item i at + i item_size), valid until destroy and
 *            read-only for the caller: what bls381_active_indices_device,
 *            bls381_proposer_indices_device and bls381_ssz_list_root_device take.
 * One thread and one stream at a time use a tree, or the caller orders them.  Host-pointer forms
 * run on the engine's own stream and return synchronised; device forms are queued on `stream`,
 * never synchronise and read nothing back to the host.  The count is kept on the host and moves
 * when an append is queued.  An update or append queues a number of launches that depends on the
 * capacity alone, never on n or n_upd.  The tree belongs to the device current at creation (calls
 * with another device current return BLS381_EARG) and holds item_size + 64 bytes per item of
 * capacity (composite) or 2 item_size (packed).  Workspaces hold *_workspace_size bytes (0 for
 * arguments the call rejects, and where the call needs none) and belong to the call.
 * BLS381_EARG: capacity 0 or above 2^31 - 1; item_size 0; a packed item_size outside the six; a
 * program bls381_ssz_root_batch would reject; a NULL argument that is needed (the tree always;
 * data and outputs when the item count is not 0; the workspace of a device form whose size
 * function is not 0); n_upd or n_idx above 2^31 - 1; in the device forms d_proofs, proof_stride
 * and d_root32 not 4-byte, d_indices not 4-byte or d_chunk_indices not 8-byte aligned.  The
 * program is copied at creation.  destroy(NULL) is a no-op; count, capacity and depth of NULL
 * are 0. */
typedef struct bls381_list_tree bls381_list_tree;
int bls381_list_tree_create(size_t capacity, size_t item_size, const uint32_t* prog, uint32_t prog_len,
                            bls381_list_tree** out);
void bls381_list_tree_destroy(bls381_list_tree* tree);
size_t bls381_list_tree_count(const bls381_list_tree* tree);
size_t bls381_list_tree_capacity(const bls381_list_tree* tree);
uint32_t bls381_list_tree_depth(const bls381_list_tree* tree);   /* d at the current count */
const uint8_t* bls381_list_tree_items_device(const bls381_list_tree* tree);
int bls381_list_tree_read(bls381_list_tree* tree, size_t first, size_t n, uint8_t* items_out);
size_t bls381_list_tree_append_workspace_size(const bls381_list_tree* tree, size_t n);
int bls381_list_tree_append(bls381_list_tree* tree, size_t n, const uint8_t* items);
int bls381_list_tree_append_device(bls381_list_tree* tree, size_t n, const uint8_t* d_items, void* d_workspace,
                                   void* stream);
size_t bls381_list_tree_update_workspace_size(const bls381_list_tree* tree, size_t n_upd);
int bls381_list_tree_update(bls381_list_tree* tree, size_t n_upd, const uint32_t* indices, size_t off, size_t len,
                            const uint8_t* values);
int bls381_list_tree_update_device(bls381_list_tree* tree, size_t n_upd, const uint32_t* d_indices, size_t off,
                                   size_t len, const uint8_t* d_values, void* d_workspace, void* stream);
int bls381_list_tree_root(bls381_list_tree* tree, int mix_length, uint8_t root[32]);
int bls381_list_tree_root_device(bls381_list_tree* tree, int mix_length, uint8_t* d_root32, void* stream);
int bls381_list_tree_proofs(bls381_list_tree* tree, size_t n_idx, const uint64_t* chunk_indices, uint8_t* proofs,
                            size_t proof_stride, uint8_t root[32]);
int bls381_list_tree_proofs_device(bls381_list_tree* tree, size_t n_idx, const uint64_t* d_chunk_indices,
                                   uint8_t* d_proofs, size_t proof_stride, uint8_t* d_root32, void* stream);

/* ---- committees: the producer of the grouped verify's d_entries ---------- */
/* get_shuffled_index (0_beacon-chain.md:860-882) for positions first .. first+count-1 of a list of
 * index_count: out[k] = shuffled(first+k), or indices[shuffled(first+k)] when indices != NULL
 * (compute_committee, :887-890: committee j of c is first = n*j/c, count = n*(j+1)/c - first;
 * indices holds index_count entries).  rounds = SHUFFLE_ROUND_COUNT (90 mainnet, 10 minimal;
 * 0..255, 0 = identity).  seed is host memory in both forms.
 * Divergence: index_count is at most 2^32 - 1 where the spec allows 2^40 -- registry entries
 * are 32-bit.  BLS381_EARG for a larger index_count, first + count > index_count, rounds > 255,
 * or a NULL seed / out / workspace with count > 0; count == 0 is BLS381_OK and runs nothing.
 * The call builds the table of all rounds * ceil(index_count / 256) source digests in the
 * workspace (32 bytes each) and then reads one bit per round and position; only a window of at
 * most ceil(index_count / 256) positions of a list of more than 2^24 - 256 hashes its own source
 * blocks instead (workspace: the pivots), where the table's build outweighs the window's
 * rounds hashes in sequence.  The device
 * form is queued on `stream`, not synchronised; d_workspace holds
 * bls381_shuffle_workspace_size(index_count, count, rounds) bytes (0 for arguments the call
 * rejects). */
size_t bls381_shuffle_workspace_size(uint64_t index_count, uint64_t count, uint32_t rounds);
int bls381_shuffle(uint64_t index_count, const uint8_t seed[32], uint32_t rounds, uint64_t first, uint64_t count,
                   const uint32_t* indices, uint32_t* out);
int bls381_shuffle_device(uint64_t index_count, const uint8_t seed[32], uint32_t rounds, uint64_t first,
                          uint64_t count, const uint32_t* d_indices, uint32_t* d_out, void* d_workspace,
                          void* stream);

/* convert_to_indexed's index sets (0_beacon-chain.md:905-917, :988-1001) for n_att attestations
 * over one shuffled list, as two groups per attestation in the order the grouped verify takes
 * them: group 2a = custody bit 0 (aggregation bit set and custody bit clear), group 2a+1 =
 * custody bit 1 (custody bit set, whatever the aggregation bit: get_attesting_indices(...,
 * custody_bitfield)), each sorted ascending.  Attestation a's committee is
 * shuffled[committee_off[a] .. + committee_len[a]) (a compute_committee result; at most 4,096 =
 * MAX_INDICES_PER_ATTESTATION members) and its two bitfields are bytes [bits_off[a],
 * bits_off[a+1]) of aggregation_bits and of custody_bits (bits_off: n_att + 1 entries).
 * The host half runs verify_bitfield (:970-982) on both bitfields -- ok[a] = 0 and two empty
 * groups when either fails -- and the popcounts: group_key_off (2 n_att + 1 entries, a host
 * output) is the h_group_key_off of bls381_registry_verify_multiple_grouped_device, d_entries its
 * d_entries, with h_call_group_off = [0, 2, 4, ...].  Entries past group_key_off[2 n_att] are not
 * written.  BLS381_EARG: a committee longer than 4,096 or outside n_shuffled, entries_cap (in
 * entries) below the member total, descending bits_off, or a NULL argument that is needed.  The
 * device form copies the bitfields into the workspace
 * (bls381_attesting_entries_workspace_size(n_att, bits_off[n_att])) and is queued on `stream`,
 * not synchronised; the host outputs are complete when it returns. */
size_t bls381_attesting_entries_workspace_size(size_t n_att, size_t bitfield_bytes);
int bls381_attesting_entries(size_t n_att, const uint32_t* committee_off, const uint32_t* committee_len,
                             const uint32_t* bits_off, const uint8_t* aggregation_bits, const uint8_t* custody_bits,
                             const uint32_t* shuffled, size_t n_shuffled, uint32_t* group_key_off, uint8_t* ok,
                             uint32_t* entries, size_t entries_cap);
int bls381_attesting_entries_device(size_t n_att, const uint32_t* h_committee_off, const uint32_t* h_committee_len,
                                    const uint32_t* h_bits_off, const uint8_t* h_aggregation_bits,
                                    const uint8_t* h_custody_bits, const uint32_t* d_shuffled, size_t n_shuffled,
                                    uint32_t* h_group_key_off, uint8_t* h_ok, uint32_t* d_entries, size_t entries_cap,
                                    void* d_workspace, void* stream);

/* ---- epoch context: active indices, their root and the proposers ---------- */
/* What the shuffle consumes, made where the validator records already are.  A validator field is
 * a little-endian uint64 at base + i * stride bytes: stride 8 is a plain array; stride 121 with
 * base = records + 88 / 96 / 113 is activation_epoch / exit_epoch / effective_balance of the
 * serialized Validator records (0_beacon-chain.md:284-298) that bls381_ssz_list_root_device hashes,
 * so one buffer of records serves the registry root and the epoch context.  Loads are 8 bytes wide
 * when base and stride are multiples of 8 and byte-wise otherwise, and none passes
 * base + (n - 1) * stride + 8.
 *
 * bls381_active_indices: get_active_validator_indices (:680-684) over n validators: the
 * ascending list of the i with activation_epoch[i] <= epoch < exit_epoch[i] (unsigned 64-bit:
 * FAR_FUTURE_EPOCH is 2^64 - 1) as uint32, their count and, when effective_balance != NULL, the
 * sum of their effective balances (else 0): get_total_balance of the active set without its floor
 * of 1.  The sum is 64-bit: it is exact while n * max balance < 2^64 and wraps above.  Entries of
 * the output past the count are not written.  The device form writes d_count_and_total[0] = count,
 * [1] = sum; d_indices has room for n entries.
 * Chaining: bls381_shuffle_device takes index_count as a host scalar, so a caller that feeds it
 * this list reads d_count_and_total[0] once per epoch -- the only host read of the chain
 * records -> active indices -> index root -> (seed on the host, 96 bytes) -> shuffle -> entries.
 *
 * bls381_active_index_root: hash_tree_root of the list as List[uint64] (:1545, an input of
 * generate_seed, :807-816): four indices per 32-byte chunk, the last chunk zero-padded, the tree
 * of depth ceil(log2(ceil(n / 4))) and mix_in_length(n).  n == 0 gives mix_in_length(zero chunk, 0).
 *
 * bls381_proposer_indices: get_beacon_proposer_index (:822-840) for n_slots slots at once.  Slot
 * k's first committee is shuffled[committee_off[k] .. + committee_len[k]) (as in
 * bls381_attesting_entries; with committees_per_slot committees a slot, committee
 * committees_per_slot * k of the epoch).  Try i looks at candidate = committee[(epoch + i) % len],
 * random_byte = SHA-256(seed || u64le(i / 32))[i % 32], and accepts when
 * effective_balance * 255 >= max_effective_balance * random_byte (the balance clamped to
 * max_effective_balance first, which leaves the verdict as it is); proposer_out[k] is the first
 * accepted candidate.  seed and the committee arrays are host memory in both forms.
 * Divergences: the search stops after 2^20 tries with 0xFFFFFFFF (a committee whose balances are
 * all 0 still accepts a try with probability 1/256 and reaches the cap with probability below
 * 2^-5900), and a try whose candidate is not below n_validators ends its slot with 0xFFFFFFFF
 * without reading a balance.
 *
 * BLS381_EARG: n or n_validators above 2^32 - 1, n_slots above 2^31 - 1, a stride below 8, a NULL
 * argument that is needed (fields, outputs and the workspace when the count of items is not 0;
 * count_out / d_count_and_total and the root always), d_indices / d_shuffled / d_proposer_out not
 * 4-byte or d_count_and_total not 8-byte aligned, a committee of length 0 or outside n_shuffled,
 * max_effective_balance of 0 or at least 2^56.  n == 0 / n_slots == 0 is BLS381_OK and runs no
 * kernel (the count is written as 0).  The device forms are queued on `stream`, not synchronised;
 * workspaces hold bls381_*_workspace_size bytes (0 for arguments the call rejects). */
size_t bls381_active_indices_workspace_size(size_t n);
int bls381_active_indices(size_t n, const uint8_t* activation_epoch, const uint8_t* exit_epoch, size_t stride,
                          uint64_t epoch, const uint8_t* effective_balance, size_t balance_stride,
                          uint32_t* indices_out, uint64_t* count_out, uint64_t* total_balance_out);
int bls381_active_indices_device(size_t n, const uint8_t* d_activation_epoch, const uint8_t* d_exit_epoch, size_t stride,
                                 uint64_t epoch, const uint8_t* d_effective_balance, size_t balance_stride,
                                 uint32_t* d_indices, uint64_t* d_count_and_total, void* d_workspace, void* stream);
size_t bls381_active_index_root_workspace_size(size_t n);
int bls381_active_index_root(size_t n, const uint32_t* indices, uint8_t root[32]);
int bls381_active_index_root_device(size_t n, const uint32_t* d_indices, uint8_t* d_root32, void* d_workspace,
                                    void* stream);
size_t bls381_proposer_indices_workspace_size(size_t n_slots);
int bls381_proposer_indices(size_t n_slots, const uint32_t* committee_off, const uint32_t* committee_len,
                            const uint32_t* shuffled, size_t n_shuffled, const uint8_t* effective_balance,
                            size_t balance_stride, size_t n_validators, const uint8_t seed[32], uint64_t epoch,
                            uint64_t max_effective_balance, uint32_t* proposer_out);
int bls381_proposer_indices_device(size_t n_slots, const uint32_t* h_committee_off, const uint32_t* h_committee_len,
                                   const uint32_t* d_shuffled, size_t n_shuffled, const uint8_t* d_effective_balance,
                                   size_t balance_stride, size_t n_validators, const uint8_t seed[32], uint64_t epoch,
                                   uint64_t max_effective_balance, uint32_t* d_proposer_out, void* d_workspace,
                                   void* stream);

/* ---- epoch rewards: votes, deltas, slashings and the hysteresis ------------ */
/* The whole-registry work of process_epoch over the records where they are (DESIGN.md section
 * 7g): process_rewards_and_penalties (0_beacon-chain.md:1389-1475), process_slashings (:1505-1524)
 * and the hysteresis of process_final_updates (:1535-1540).  All results are the spec's integers.
 * Validator fields are little-endian uint64 at base + i * stride as in the epoch context (one
 * `stride` for all uint64 fields of a call: 121 with bases records + 88 / 96 / 104 / 113 for
 * activation_epoch / exit_epoch / withdrawable_epoch / effective_balance, or 8 over plain arrays);
 * the slashed flag is one byte at slashed + i * slashed_stride (records + 112 with stride 121, or
 * stride 1 over a plain array; any non-zero byte is slashed).  Balances, rewards, penalties and
 * values are plain uint64 arrays, 8-byte aligned.
 *
 * bls381_epoch_votes: the PendingAttestations of one epoch (previous or current) as per-validator
 * facts and per-committee crosslink results.  Committee c is shuffled[committee_off[c] .. +
 * committee_len[c]) (at most 4,096 members; the slices lie inside n_shuffled and do not overlap,
 * and the shuffled list is a permutation, so a validator sits in at most one committee).  Its
 * attestations are att_off[c] .. att_off[c+1] - 1 (n_committees + 1 entries, n_att =
 * att_off[n_committees]), in the order they have in the state list.  Attestation a has its
 * aggregation bitfield at bytes [bits_off[a], bits_off[a+1]) of aggregation_bits, att_flags[a]
 * (bit 0: matching target, bit 1: matching head; the caller has compared the roots),
 * att_inclusion_delay[a], att_proposer[a] and att_candidate[a]: 0 .. cand_count[c] - 1, the
 * crosslink candidate of its committee it votes for, or 0xFFFFFFFF for none.  The host half runs
 * verify_bitfield (:970-982) on every bitfield.  Outputs:
 *   votes[i]           bit 0: i attests in some attestation (source), bit 1: in one with the
 *                      target flag, bit 2: in one with the head flag, bit 3: in an attestation of
 *                      its committee's winning candidate, bit 4: member of a committee.  Bits 0-3
 *                      only for slashed == 0 (get_unslashed_attesting_indices, :1294-1300); 0 for
 *                      a validator in no committee.  All n_validators words are written.
 *   incl_delay[i], incl_proposer[i]   for i with bit 0: inclusion_delay and proposer_index of the
 *                      attestation min(..., key=inclusion_delay) picks (:1424-1427): the smallest
 *                      delay, among equals the first in list order.  Other entries are not written.
 *   committee_of[i]    i's committee, or 0xFFFFFFFF.  All n_validators words are written.
 *   winner[c], winner_balance[c], committee_balance[c]   the candidate with the largest attesting
 *                      balance (the sum of effective_balance over the unslashed members of the
 *                      union of its attestations), among equals the largest id, or 0xFFFFFFFF with
 *                      balance 0 when cand_count[c] == 0; the sum over all members.  Unfloored.
 *   totals[0..2]       the sums of effective_balance over the validators with bit 0, 1 and 2:
 *                      get_attesting_balance of the matching source / target / head attestations
 *                      without its floor of 1.  64-bit sums.
 * A member at or above n_validators is passed over.  The device form takes the committee and
 * attestation arrays as host memory and the shuffled list and the fields as device memory, copies
 * the descriptors and bitfields into the workspace (bls381_epoch_votes_workspace_size(
 * n_committees, n_att, bits_off[n_att])) and writes d_totals (3 entries).
 *
 * bls381_epoch_deltas: get_attestation_deltas (which & 1) and get_crosslink_deltas (which & 2)
 * over the outputs of bls381_epoch_votes for the previous epoch, and their application:
 * rewards[i] and penalties[i] are the sums of the chosen kinds, new_balances[i] =
 * decrease_balance(increase_balance(balances[i], rewards[i]), penalties[i]) (saturating at 0);
 * new_balances may be balances.  total_balance is get_total_active_balance of the current epoch
 * (floored at 1 here); in the device form it is a device pointer, d_count_and_total + 1 of
 * bls381_active_indices_device, and the host reads nothing back.  integer_squareroot is computed
 * on the device, exactly.  eligible = active at previous_epoch, or slashed with previous_epoch + 1
 * < withdrawable_epoch; the inclusion rewards go to every validator with bit 0; the inactivity
 * branch runs when previous_epoch - finalized_epoch > min_epochs_to_inactivity_penalty.
 * Overflows: products go through a 128-bit product; a quotient of 2^64 or more, a per-validator
 * sum that wraps and an increase_balance that wraps saturate at 2^64 - 1 and each adds 1 to the
 * status word; a proposer micro-reward of 2^32 or more, an incl_proposer at or above n, an
 * incl_delay of 0 (with bit 0) and a committee_of at or above n_committees (other than
 * 0xFFFFFFFF) add nothing and each adds 1.  The host form returns the count in *overflows_out;
 * the device form zeroes and then counts in *d_status (uint64).  Workspace:
 * bls381_epoch_deltas_workspace_size(n).
 *
 * bls381_epoch_slashings: process_slashings over balances in place: for slashed validators with
 * current_epoch == withdrawable_epoch - latest_slashed_exit_length / 2 the penalty
 * max(effective_balance * min(3 total_penalties, total_balance) / total_balance,
 * effective_balance / min_slashing_penalty_quotient), none of whose terms wraps; total_penalties
 * is the caller's difference of latest_slashed_balances, total_balance as above.
 *
 * bls381_effective_balances: the hysteresis.  indices[i] = i where validator i's effective
 * balance changes (balance < effective_balance or effective_balance + 3 (increment / 2) <
 * balance, compared without wrapping, and the new value min(balance - balance % increment,
 * max_effective_balance) differs) and 0xFFFFFFFF where it does not; values[i] = the new (or
 * unchanged) value; *changed = how many changed.  bls381_list_tree_update_device takes the two
 * arrays as they are (off = 113, len = 8, n_upd = n): it skips 0xFFFFFFFF.
 *
 * BLS381_EARG: n, n_validators or n_shuffled above 2^32 - 1, n_committees or n_att above 2^31 - 1;
 * a stride below 8 or a slashed_stride of 0; a NULL argument that is needed (fields, inputs and
 * outputs when the count of items is not 0; constants, total_balance, overflows_out / d_status,
 * changed_out / d_changed and d_totals always; the workspace of a device form whose size is not
 * 0); uint64 arrays not 8-byte or uint32 arrays not 4-byte aligned in the device forms; a
 * committee longer than 4,096, outside n_shuffled or overlapping another; descending att_off or
 * bits_off; a bitfield that fails verify_bitfield; att_flags above 3; a candidate that is neither
 * 0xFFFFFFFF nor below its committee's cand_count; which outside 1..3; previous_epoch of 2^64 - 1
 * or below finalized_epoch; base_rewards_per_epoch, proposer_reward_quotient,
 * inactivity_penalty_quotient, min_slashing_penalty_quotient or increment of 0.  A count of 0 is
 * BLS381_OK and runs no kernel (the scalar outputs are written as 0).  Host-pointer forms stage,
 * run on the engine's stream and return synchronised; device forms are queued on `stream`, never
 * synchronise and read nothing back. */
typedef struct bls381_reward_constants {
  uint64_t base_reward_factor;
  uint64_t base_rewards_per_epoch;
  uint64_t proposer_reward_quotient;
  uint64_t min_attestation_inclusion_delay;
  uint64_t min_epochs_to_inactivity_penalty;
  uint64_t inactivity_penalty_quotient;
} bls381_reward_constants;
size_t bls381_epoch_votes_workspace_size(size_t n_committees, size_t n_att, size_t bitfield_bytes);
int bls381_epoch_votes(size_t n_committees, const uint32_t* committee_off, const uint32_t* committee_len,
                       const uint32_t* shuffled, size_t n_shuffled, size_t n_validators, const uint8_t* slashed,
                       size_t slashed_stride, const uint8_t* effective_balance, size_t stride, const uint32_t* att_off,
                       const uint32_t* bits_off, const uint8_t* aggregation_bits, const uint8_t* att_flags,
                       const uint64_t* att_inclusion_delay, const uint32_t* att_proposer, const uint32_t* att_candidate,
                       const uint32_t* cand_count, uint32_t* votes, uint64_t* incl_delay, uint32_t* incl_proposer,
                       uint32_t* committee_of, uint32_t* winner, uint64_t* winner_balance, uint64_t* committee_balance,
                       uint64_t totals[3]);
int bls381_epoch_votes_device(size_t n_committees, const uint32_t* h_committee_off, const uint32_t* h_committee_len,
                              const uint32_t* d_shuffled, size_t n_shuffled, size_t n_validators,
                              const uint8_t* d_slashed, size_t slashed_stride, const uint8_t* d_effective_balance,
                              size_t stride, const uint32_t* h_att_off, const uint32_t* h_bits_off,
                              const uint8_t* h_aggregation_bits, const uint8_t* h_att_flags,
                              const uint64_t* h_att_inclusion_delay, const uint32_t* h_att_proposer,
                              const uint32_t* h_att_candidate, const uint32_t* h_cand_count, uint32_t* d_votes,
                              uint64_t* d_incl_delay, uint32_t* d_incl_proposer, uint32_t* d_committee_of,
                              uint32_t* d_winner, uint64_t* d_winner_balance, uint64_t* d_committee_balance,
                              uint64_t* d_totals, void* d_workspace, void* stream);
size_t bls381_epoch_deltas_workspace_size(size_t n);
int bls381_epoch_deltas(size_t n, const uint8_t* activation_epoch, const uint8_t* exit_epoch,
                        const uint8_t* withdrawable_epoch, const uint8_t* effective_balance, size_t stride,
                        const uint8_t* slashed, size_t slashed_stride, const uint32_t* votes, const uint64_t* incl_delay,
                        const uint32_t* incl_proposer, const uint32_t* committee_of, size_t n_committees,
                        const uint64_t* winner_balance, const uint64_t* committee_balance, const uint64_t totals[3],
                        const uint64_t* balances, uint64_t previous_epoch, uint64_t finalized_epoch,
                        uint64_t total_balance, const bls381_reward_constants* constants, uint32_t which,
                        uint64_t* rewards, uint64_t* penalties, uint64_t* new_balances, uint64_t* overflows_out);
int bls381_epoch_deltas_device(size_t n, const uint8_t* d_activation_epoch, const uint8_t* d_exit_epoch,
                               const uint8_t* d_withdrawable_epoch, const uint8_t* d_effective_balance, size_t stride,
                               const uint8_t* d_slashed, size_t slashed_stride, const uint32_t* d_votes,
                               const uint64_t* d_incl_delay, const uint32_t* d_incl_proposer,
                               const uint32_t* d_committee_of, size_t n_committees, const uint64_t* d_winner_balance,
                               const uint64_t* d_committee_balance, const uint64_t* d_totals, const uint64_t* d_balances,
                               uint64_t previous_epoch, uint64_t finalized_epoch, const uint64_t* d_total_balance,
                               const bls381_reward_constants* constants, uint32_t which, uint64_t* d_rewards,
                               uint64_t* d_penalties, uint64_t* d_new_balances, uint64_t* d_status, void* d_workspace,
                               void* stream);
int bls381_epoch_slashings(size_t n, const uint8_t* slashed, size_t slashed_stride, const uint8_t* withdrawable_epoch,
                           const uint8_t* effective_balance, size_t stride, uint64_t current_epoch,
                           uint64_t total_penalties, uint64_t total_balance, uint64_t latest_slashed_exit_length,
                           uint64_t min_slashing_penalty_quotient, uint64_t* balances);
int bls381_epoch_slashings_device(size_t n, const uint8_t* d_slashed, size_t slashed_stride,
                                  const uint8_t* d_withdrawable_epoch, const uint8_t* d_effective_balance, size_t stride,
                                  uint64_t current_epoch, uint64_t total_penalties, const uint64_t* d_total_balance,
                                  uint64_t latest_slashed_exit_length, uint64_t min_slashing_penalty_quotient,
                                  uint64_t* d_balances, void* stream);
int bls381_effective_balances(size_t n, const uint64_t* balances, const uint8_t* effective_balance, size_t stride,
                              uint64_t increment, uint64_t max_effective_balance, uint32_t* indices, uint64_t* values,
                              uint64_t* changed_out);
int bls381_effective_balances_device(size_t n, const uint64_t* d_balances, const uint8_t* d_effective_balance,
                                     size_t stride, uint64_t increment, uint64_t max_effective_balance,
                                     uint32_t* d_indices, uint64_t* d_values, uint64_t* d_changed, void* stream);

/* ---- registry updates: ejections, the exit queue and the activation queue --- */
/* process_registry_updates (0_beacon-chain.md:1480-1502) with initiate_validator_exit (:1110-1128)
 * and get_churn_limit (:1081-1088) over the records where they are.  Validator
 * fields are little-endian uint64 at base + i * stride as above, one `stride` for the five fields of
 * a call: 121 with bases records + 80 / 88 / 96 / 104 / 113 for activation_eligibility_epoch /
 * activation_epoch / exit_epoch / withdrawable_epoch / effective_balance, or 8 over plain arrays.
 * With FAR = 2^64 - 1, cur = current_epoch and delayed(e) = e + 1 + activation_exit_delay:
 *   eligibility   activation_eligibility_epoch becomes cur where it is FAR and effective_balance >=
 *                 max_effective_balance.
 *   ejections     a validator active at cur (activation_epoch <= cur < exit_epoch) with
 *                 effective_balance <= ejection_balance and exit_epoch == FAR leaves through the exit
 *                 queue: with L = max(min_per_epoch_churn_limit, active count /
 *                 churn_limit_quotient), E0 = the largest exit_epoch != FAR in the registry or
 *                 delayed(cur), whichever is larger, and c0 = how many validators hold E0, the k-th
 *                 ejected validator in index order (k from 0) gets exit_epoch = E0 + (min(c0, L) + k)
 *                 / L and withdrawable_epoch = exit_epoch + min_validator_withdrawability_delay.
 *   activations   the candidates (eligibility != FAR after the first step, activation_epoch >=
 *                 delayed(finalized_epoch)) in the order of (eligibility, index); the first L of
 *                 them are dequeued, and a dequeued one whose activation_epoch is FAR gets
 *                 delayed(cur).  One that already has an activation epoch takes a place and keeps it.
 * These are the spec's loops in closed form; every result is the spec's integer.
 *
 * bls381_registry_updates: indices[i] = i where any of validator i's four epochs changes and
 * 0xFFFFFFFF where none does; values[32 i ..] = activation_eligibility_epoch, activation_epoch,
 * exit_epoch, withdrawable_epoch, new or old, as four little-endian uint64.
 * bls381_list_tree_update_device takes the two arrays as they are (off = 80, len = 32, n_upd = n).
 * summary: [0] eligibilities set, [1] validators ejected, [2] validators activated, [3] validators
 * changed, [4] the active count at cur, [5] L, [6] E0 before the call, [7] the status word.  An
 * exit_epoch or withdrawable_epoch that would pass 2^64 - 1 becomes 2^64 - 1 and its validator adds
 * 1 to the status word.  n == 0 writes the summary alone (E0 = delayed(cur), L = the minimum).
 *
 * bls381_exit_queue: initiate_validator_exit's view of the registry (:1119-1124): queue[0] = E0,
 * [1] = c0, [2] = L, [3] = the active count.  The next exit gets E0 + (min(c0, L) + k) / L with k
 * the exits the caller has made since, so a block's voluntary exits and slashings are arithmetic.
 * The device form has no status word: where the data gives no churn limit (see below) it writes
 * queue[2] = 0 and returns BLS381_OK, so its caller checks queue[2] before dividing by it.
 *
 * BLS381_EARG: n above 2^32 - 1; a stride below 8; a NULL argument that is needed (fields, indices
 * and values when n is not 0; constants, summary / d_summary, queue / d_queue and the workspace
 * always); d_indices not 4-byte or d_values, d_summary, d_queue not 8-byte aligned;
 * churn_limit_quotient of 0; current_epoch + 1 + activation_exit_delay or finalized_epoch + 1 +
 * activation_exit_delay at or above 2^64; min_per_epoch_churn_limit of 0 with n <
 * churn_limit_quotient.  A churn limit of 0 that only the data shows (min_per_epoch_churn_limit of 0
 * and fewer than churn_limit_quotient active validators) is BLS381_EARG in the host forms, which
 * then write nothing; the device forms cannot know: they report no change for every validator, L =
 * 0, and bit 63 of the status word set.  Host-pointer forms stage, run on the engine's stream and
 * return synchronised; device forms are queued on `stream`, never synchronise and read nothing
 * back.  The workspace holds bls381_registry_updates_workspace_size(n) bytes (both calls; never 0
 * for n up to 2^32 - 1). */
typedef struct bls381_registry_constants {
  uint64_t max_effective_balance;
  uint64_t ejection_balance;
  uint64_t activation_exit_delay;
  uint64_t min_validator_withdrawability_delay;
  uint64_t min_per_epoch_churn_limit;
  uint64_t churn_limit_quotient;
} bls381_registry_constants;
size_t bls381_registry_updates_workspace_size(size_t n);
int bls381_registry_updates(size_t n, const uint8_t* activation_eligibility_epoch, const uint8_t* activation_epoch,
                            const uint8_t* exit_epoch, const uint8_t* withdrawable_epoch, const uint8_t* effective_balance,
                            size_t stride, uint64_t current_epoch, uint64_t finalized_epoch,
                            const bls381_registry_constants* constants, uint32_t* indices, uint8_t* values,
                            uint64_t summary[8]);
int bls381_registry_updates_device(size_t n, const uint8_t* d_activation_eligibility_epoch,
                                   const uint8_t* d_activation_epoch, const uint8_t* d_exit_epoch,
                                   const uint8_t* d_withdrawable_epoch, const uint8_t* d_effective_balance, size_t stride,
                                   uint64_t current_epoch, uint64_t finalized_epoch,
                                   const bls381_registry_constants* constants, uint32_t* d_indices, uint8_t* d_values,
                                   uint64_t* d_summary, void* d_workspace, void* stream);
int bls381_exit_queue(size_t n, const uint8_t* activation_epoch, const uint8_t* exit_epoch, size_t stride,
                      uint64_t current_epoch, const bls381_registry_constants* constants, uint64_t queue[4]);
int bls381_exit_queue_device(size_t n, const uint8_t* d_activation_epoch, const uint8_t* d_exit_epoch, size_t stride,
                             uint64_t current_epoch, const bls381_registry_constants* constants, uint64_t* d_queue,
                             void* d_workspace, void* stream);

/* ---- fork choice: latest messages and the LMD-GHOST head ------------------- */
/* lmd_ghost (0_fork-choice.md:78-103) with get_ancestor (:56-69) and the latest-attestation rule
 * (:71-72) over a store that keeps the block tree on the host and one latest message per validator
 * on the device.  One thread and one stream at a time use a store, or the
 * caller orders them.  The store belongs to the device current at creation and holds 12 bytes per
 * validator of validator_capacity and 80 bytes per block of block_capacity there.
 *
 * Blocks.  add_blocks appends n blocks (32-byte roots, 32-byte parent roots, slots) and writes their
 * node ids to node_out (may be NULL).  The first block ever added is the anchor: its parent root is
 * not looked at.  Ids are dense in insertion order, so a parent's id is below its children's.  A
 * root that is already known returns the id it has.  BLS381_EARG, and no block of the call is
 * added: an unknown parent, a slot not above the parent's, a slot at or above 2^32, more blocks
 * than block_capacity.  node looks a root up (0xFFFFFFFF: unknown), root gives a node's root,
 * block_count the number of nodes.
 *
 * Latest messages.  A message is the key (slot << 32) | (0xFFFFFFFF - seq) and a target node
 * (0xFFFFFFFF: none); seq numbers the attestations over the life of the store in the order they
 * were handed in, and the larger key wins: the highest slot, and among equal slots the attestation
 * handed in first.  Slots and seq stay below 2^32: a slot at or above 2^32, or an attestation that
 * would be number 2^32 - 1 or later, is BLS381_EARG.
 * on_attestations: attestation a (slot slots[a], target node target_nodes[a]) has the validators
 * entries[att_off[a] .. att_off[a+1]) as members (att_off: n_att + 1 ascending entries).  With the
 * arrays of bls381_attesting_entries_device, att_off[a] = group_key_off[2 a] and d_entries goes in
 * as it is.  att_off, slots and target_nodes are host memory in both forms; entries and ok are
 * device memory in the _device form.  ok may be NULL; else the members of an attestation with
 * ok[a] == 0 (a verdict of the grouped verify, which the device form reads when the kernels run)
 * are not looked at, and the attestation still takes its seq.  A member at or above
 * validator_capacity is skipped and counted in *skipped (written by the call; the device form
 * writes d_skipped).  The result does not depend on the order in which the device visits members.
 * BLS381_EARG, and nothing changes: descending att_off, a target node that is not in the tree, the
 * slot and seq bounds above, a NULL argument that is needed (the store and skipped always; the
 * three host arrays when n_att is not 0; entries and the workspace when there are members),
 * d_entries not 4-byte or d_skipped not 8-byte aligned.  The workspace holds
 * bls381_fork_choice_on_attestations_workspace_size(n_att) bytes (0 above 2^32 - 1 attestations).
 * read_latest: slots_out[k] = the slot of validator first + k's message (0 when it never had one),
 * targets_out[k] its target node.  first + n above validator_capacity is BLS381_EARG.
 *
 * prune(new_anchor_node): the subtree of that node stays, renumbered in insertion order (the new
 * anchor is node 0), the rest of the tree goes; a message whose target went keeps its key and gets
 * target none.  Waits for the device, runs one pass over the messages, returns synchronised.
 *
 * head: validator i < n votes with effective_balance[i] for its target when activation_epoch[i] <=
 * epoch < exit_epoch[i] and it has a message.  The fields are little-endian uint64 at base + i *
 * stride as in the epoch context (121 with bases records + 88 / 96 / 113, or 8 over plain arrays);
 * they are the columns of the start state, which for the spec's head is the justified state.  A
 * block's vote count is the sum of the votes whose target is the block or a descendant
 * (get_ancestor(target, block.slot) == block).  The head is reached from start_node by taking the
 * child with the largest (vote count, root as a byte string) until a node has no child.
 * head_out / d_head_out: the head's node id; head_root32 (host form, may be NULL): its root;
 * weights_out / d_weights_out (may be NULL): the vote count of every node, block_count entries;
 * status_out / d_status_out: one word, the number of nodes whose vote count would pass 2^64 - 1
 * and reads 2^64 - 1.  Fields of validators without a message are not read.
 * BLS381_EARG, and nothing is written: start_node not in the tree, n above validator_capacity, a
 * stride below 8, a NULL argument that is needed (the store, head_out and status_out always; the
 * fields when n is not 0), d_head_out not 4-byte or d_weights_out / d_status_out not 8-byte aligned.
 * The device form queues a number of launches that depends on block_capacity alone (its
 * ceil(log2(block_capacity)) rounds of pointer doubling), uploads the tree's numbering when the tree
 * has changed since the last head, never synchronises and reads nothing back.  The host forms
 * stage, run on the engine's stream and return synchronised. */
typedef struct bls381_fork_choice bls381_fork_choice;
int bls381_fork_choice_create(size_t validator_capacity, size_t block_capacity, bls381_fork_choice** out);
void bls381_fork_choice_destroy(bls381_fork_choice* fc);
int bls381_fork_choice_add_blocks(bls381_fork_choice* fc, size_t n, const uint8_t* roots32, const uint8_t* parent_roots32,
                                  const uint64_t* slots, uint32_t* node_out);
uint32_t bls381_fork_choice_node(const bls381_fork_choice* fc, const uint8_t root32[32]);
int bls381_fork_choice_root(const bls381_fork_choice* fc, uint32_t node, uint8_t root32[32]);
size_t bls381_fork_choice_block_count(const bls381_fork_choice* fc);
size_t bls381_fork_choice_on_attestations_workspace_size(size_t n_att);
int bls381_fork_choice_on_attestations(bls381_fork_choice* fc, size_t n_att, const uint32_t* att_off, const uint32_t* entries,
                                       const uint64_t* slots, const uint32_t* target_nodes, const uint8_t* ok,
                                       uint64_t* skipped_out);
int bls381_fork_choice_on_attestations_device(bls381_fork_choice* fc, size_t n_att, const uint32_t* h_att_off,
                                              const uint32_t* d_entries, const uint64_t* h_slots,
                                              const uint32_t* h_target_nodes, const uint8_t* d_ok, uint64_t* d_skipped,
                                              void* d_workspace, void* stream);
int bls381_fork_choice_read_latest(bls381_fork_choice* fc, size_t first, size_t n, uint64_t* slots_out,
                                   uint32_t* targets_out);
int bls381_fork_choice_prune(bls381_fork_choice* fc, uint32_t new_anchor_node);
int bls381_fork_choice_head(bls381_fork_choice* fc, uint32_t start_node, size_t n, const uint8_t* activation_epoch,
                            const uint8_t* exit_epoch, const uint8_t* effective_balance, size_t stride, uint64_t epoch,
                            uint32_t* head_out, uint8_t head_root32[32], uint64_t* weights_out, uint64_t* status_out);
int bls381_fork_choice_head_device(bls381_fork_choice* fc, uint32_t start_node, size_t n, const uint8_t* d_activation_epoch,
                                   const uint8_t* d_exit_epoch, const uint8_t* d_effective_balance, size_t stride,
                                   uint64_t epoch, uint32_t* d_head_out, uint64_t* d_weights_out, uint64_t* d_status_out,
                                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BLS381_H */
