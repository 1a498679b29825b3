/*
 * mpshuffle.h -- C ABI of libmpshuffle.so: the MI355X (gfx950) shuffle-proof engine that replaces, for the
 * hot path only, the `BarnettSmartProtocol` implementation of geometryxyz/mental-poker:
 *
 *     DLCards::setup               [REF barnett-smart-card-protocol/src/discrete_log_cards/mod.rs:105-121]
 *     DLCards::shuffle_and_remask  [REF .../discrete_log_cards/mod.rs:380-418, trait decl src/lib.rs:181-188]
 *     DLCards::verify_shuffle      [REF .../discrete_log_cards/mod.rs:420-443, trait decl src/lib.rs:191-197]
 *
 * The reference has no FFI seam -- its seam is the Rust trait (a second `impl BarnettSmartProtocol`); these are
 * the entry points such an impl binds through `extern "C"` (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - plain pointers and sizes; the CALLER allocates every buffer (sizes: mp_proof_size, mp_params_size);
 *   - all multi-byte buffers must be 4-byte aligned;
 *   - return value / status word: 0 = Ok; > 0 = proof rejected, value = code of the first failing check
 *     (mp_check_name: 1 "Hadamard Product (5.1)" [REF tests.rs:223-225], 2 "Zero Argument (5.2)",
 *     3 "Single Value Product (5.3)", 4 "Multi-Exponentiation Argument (4)") <-> CryptoError::ProofVerificationError;
 *     < 0 = usage / encoding error <-> CardProtocolError::IoError [REF src/error.rs:6-12]
 *     (MP_ERR_*; text via mp_last_error);
 *   - wire encodings ("mpshuffle wire v1"):
 *       scalar (Fr)      32 B little-endian canonical integer, must be < group order
 *       point            mp_point_size(curve) B: x LE || y LE (canonical, affine), 8 bytes per ark-ff limb of the base
 *                        field: 64 B on the 256-bit curves, 96 B on BLS12-377; point at infinity = all-zero bytes
 *       ciphertext/card  two points: c0 || c1                             (el_gamal::Ciphertext(pub Affine, pub Affine))
 *       deck             N ciphertexts back to back, N = m*n
 *       parameters       (n+3) points: G | ck_0 .. ck_{n-1} | H | gen     (enc generator, Pedersen key, extra generator)
 *       permutation      N uint32, out[i] = in[perm[i]]                   (Permutation::permute_array)
 *       proof            mp_proof_size(m, n) bytes, element order in DESIGN.md ("proof wire order")
 *   - prover randomness is an explicit 32-byte seed: the prover draws `Fr::rand` from
 *     ChaCha20Rng::from_seed(seed) in the documented order (the reference takes `rng: &mut R`, mod.rs:381).
 *   - thread-safety (round 6; the reference's trait members are associated functions without `self` or global state [REF src/lib.rs:74-197],
 *     so any number of host threads may prove and verify at once): every entry point that takes a context, a table or a key set holds
 *     the CONTEXT's lock for the length of the call.  Calls from several host threads on one context (or on tables of one context) are
 *     therefore safe and run one after the other, in the order the threads get the lock -- a prove or verify call of 2 048 proofs is a few
 *     milliseconds; calls on DIFFERENT contexts share nothing (streams, arenas, tables and profiler are per context) and run side by
 *     side on the device.  mp_last_error is per thread.  What stays with the caller: a buffer handed to a call is not written by
 *     another thread until the call has returned (pipelined verification, mp_set_pipeline: until mp_sync or `depth` further verify
 *     calls have), and no call is in flight on a context or table that is being destroyed.  The library reads no environment variable
 *     and keeps no mutable global.  tests/test_gpu_round6.py::test_four_host_threads_* and tests/test_threads_tsan.py hold it to that.
 *     Coalescing (mp_set_coalesce, off by default): the single-proof calls of several threads on one table are gathered into batched
 *     calls; a thread still gets only its own outputs, status word and mp_last_error.  mp_set_coalesce applies to the batches opened
 *     after it -- a batch already open completes under the settings it opened with -- and may be called at any time, also while
 *     calls are queued.  mp_table_destroy while single-proof calls are queued or in flight on that table is the caller's error, as for
 *     every other call.  tests/test_coalesce_tsan.py and tests/test_gpu_coalesce.py hold it to that.
 */
#ifndef MPSHUFFLE_H
#define MPSHUFFLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MP_CURVE_STARK 0      /* starknet_curve::Projective: every reference test + examples/round.rs */
#define MP_CURVE_BN254 1
#define MP_CURVE_SECP256K1 2
#define MP_CURVE_BLS12_377 3  /* ark_bls12_377::G1Projective: examples/parameter_selection.rs [REF :25] (377-bit base field) */

#define MP_OK 0
#define MP_ERR_BAD_ENCODING (-1)     /* non-canonical scalar / coordinate, point not on the curve */
#define MP_ERR_BAD_PERMUTATION (-2)
#define MP_ERR_BAD_ARGUMENT (-3)     /* null pointer, m < 2, n < 2, N > 4096, wrong proof length ... */
#define MP_ERR_NO_DEVICE (-4)        /* no usable MI355X / HIP runtime error: the engine never falls back to a CPU path */
#define MP_ERR_INTERNAL (-5)

typedef struct mp_ctx mp_ctx;       /* one GPU + stream + curve */
typedef struct mp_table mp_table;   /* shared parameters + shared key of one card table, with their device tables */

/* ---- context ---------------------------------------------------------------------------------------- */
int mp_ctx_create(int curve_id, int device, mp_ctx** out);
void mp_ctx_destroy(mp_ctx* ctx);                 /* tables of the context that are still alive keep it alive: it goes with the last of them */
const char* mp_last_error(void);                 /* thread-local text of the last error */
const char* mp_check_name(int code);             /* "Ok", "Hadamard Product (5.1)", ... */
size_t mp_proof_size(uint32_t m, uint32_t n);    /* (11m+8) points + (5n+9) scalars, 64-byte points (the 256-bit curves) */
size_t mp_params_size(uint32_t n);               /* (n+3) * 64 */
size_t mp_point_size(int curve_id);                              /* wire bytes of one point: 64, or 96 on MP_CURVE_BLS12_377 */
size_t mp_proof_size_curve(int curve_id, uint32_t m, uint32_t n); /* same counts with mp_point_size(curve_id) per point */
size_t mp_params_size_curve(int curve_id, uint32_t n);            /* (n+3) * mp_point_size(curve_id) */

/* Page-locked host memory for the host-buffer entry points (mp_*_batch): with buffers from mp_host_alloc every transfer is
 * an asynchronous DMA that overlaps the kernels of the neighbouring chunks; ordinary (pageable) buffers work too, at the
 * runtime's staging speed.  NULL on failure (mp_last_error). */
void* mp_host_alloc(size_t bytes);
void mp_host_free(void* p);
/* proofs per pipelined chunk of the host-buffer entry points (0 restores the default: 65 536, and 131 072 for calls of 262 144 proofs or
 * more; the first chunks of a call are smaller -- the first upload and the last download are the copies nothing overlaps -- and the chunks
 * of a verify call grow by half from one to the next, because the copy of chunk k + 1 takes about as long as the kernels of chunk k) */
int mp_set_io_chunk(mp_table* t, size_t proofs);
/* The chunks a host-buffer call of B proofs takes on this table under its current mp_set_io_chunk, in order: those of a prove call
 * (mp_shuffle_and_remask_batch, its _keys and _seeded forms; verify = 0) or of a verify call (mp_verify_shuffle_batch[_keys]; verify != 0).
 * Returns their number and writes the first `cap` sizes to out_chunks (which may be NULL when cap is 0); the sizes sum to B, none is 0 and
 * none exceeds min(B, chunk).  Read-only: it starts no device work, and it is computed by the code the calls themselves cut their batch
 * with.  0 for a NULL table or B = 0. */
size_t mp_io_schedule(const mp_table* t, size_t B, int verify, size_t* out_chunks, size_t cap);

/* ---- DLCards::setup [REF barnett-smart-card-protocol/src/discrete_log_cards/mod.rs:105-121] ---------------------------
 * "setup v2": G, ck_0..ck_{n-1}, H, gen -- n + 3 INDEPENDENT curve points sampled the way ark-ec's `C::rand` does from
 * ChaCha20Rng::from_seed(seed), in that order: x = Fq::rand, a sign bit, the square root of x^3 + a x + b (retry if there is none),
 * cofactor cleared.  Nobody, the holder of the seed included, knows a discrete logarithm between two of them (round 1 derived
 * them as k * G_std, which made the seed a trapdoor of the Pedersen key).  Host work, once per table.  out_params: n + 3 wire points. */
int mp_setup(mp_ctx* ctx, uint32_t m, uint32_t n, const uint8_t seed[32], uint8_t* out_params);

/* ---- table context: Parameters + aggregate public key -> fixed-base window tables in HBM ------------------
 * mp_table_create sizes the tables for the GPU it runs on: the widest windows -- 21 bits (48 GB at n = 26, 12 additions per term on the
 * 252-bit STARK scalars), 20 (27 GB, 13 additions), 16 (2 GB, 16 additions), 8 (16 MB, 32 additions) -- whose tables take at most 30 % of
 * the HBM that is free at the call and whose construction (~3.3x the table for a moment) fits 85 % of it.  On an otherwise empty
 * MI355X that is the configuration bench.py measures; a caller that keeps many tables alive (one per aggregate key) should rather
 * create ONE table of the shared parameters and name the keys through a key set (below).  Construction takes 0.1 s (8 / 16 bits) to
 * ~3 s (21 bits, first touch of 150 GB). */
int mp_table_create(mp_ctx* ctx, uint32_t m, uint32_t n, const uint8_t* params, const uint8_t* shared_key,
                    mp_table** out);
/* same with an explicit fixed-base window width: 8, 16, 20 or 21 bits (21: ceil(scalar bits / 21) windows -- 12 on the STARK curve, 13
 * on the other curves, where 20 bits give the same count for half the memory); 0 = choose as mp_table_create does */
int mp_table_create_ex(mp_ctx* ctx, uint32_t m, uint32_t n, const uint8_t* params, const uint8_t* shared_key,
                       uint32_t fb_window_bits, mp_table** out);
uint32_t mp_table_window_bits(const mp_table* t);      /* the width in use */
void mp_table_destroy(mp_table* t);

/* ---- DLCards::shuffle_and_remask / verify_shuffle (one proof; host buffers) --------------------------------- */
/* prover_seed: 32 FRESH uniformly random bytes per proof.  It stands for the reference's `rng: &mut R` [REF src/lib.rs:181-188]
 * and keys the ChaCha20 stream behind every blinding value of the argument; like any sigma-type proof, two proofs made from
 * one seed with different witnesses reveal the witnesses (permutation and masking factors).  (The sigma protocols further
 * down hedge their single nonce with witness and statement; the shuffle prover draws its O(N) blinders from the seed alone.) */
int mp_shuffle_and_remask(mp_table* t, const uint8_t* deck, const uint8_t* masking_factors,
                          const uint32_t* permutation, const uint8_t prover_seed[32], uint8_t* out_deck,
                          uint8_t* out_proof);
int mp_verify_shuffle(mp_table* t, const uint8_t* deck, const uint8_t* shuffled_deck, const uint8_t* proof,
                      size_t proof_len);
/* the same with the aggregate key given per call, as the reference passes `shared_key` [REF mod.rs:380-386, 420-426]: valid on keyless
 * tables (mp_table_create_params) and on keyed ones, whose own key it overrides for this call.  Bytes and status words are those of
 * mp_shuffle_and_remask / mp_verify_shuffle on a table created with that key. */
int mp_shuffle_and_remask_keyed(mp_table* t, const uint8_t* shared_key, const uint8_t* deck, const uint8_t* masking_factors,
                                const uint32_t* permutation, const uint8_t prover_seed[32], uint8_t* out_deck, uint8_t* out_proof);
int mp_verify_shuffle_keyed(mp_table* t, const uint8_t* shared_key, const uint8_t* deck, const uint8_t* shuffled_deck,
                            const uint8_t* proof, size_t proof_len);
/* Coalescing of the four single-proof entry points above (off by default: every call is a batch of one).  A server with many
 * concurrent single-proof requests sets it on ONE table (a keyless one with the _keyed calls, when its card tables differ by key):
 * the calls that arrive while the context is busy are gathered and each gathering is ONE batched call (mp_*_batch / mp_*_batch_keys),
 * so T threads share the throughput of a batch of ~T proofs instead of running T batches of one.  Four queues per table -- prove and
 * verify, each with and without a per-call key -- that never mix.  A batch closes when it holds max_batch requests (1 .. 65 536), or
 * when its first caller holds the context's lock and max_wait_us have passed since it opened (0: a lone caller on an idle context
 * waits for nothing; while an earlier batch runs, the next one fills by itself).  Every caller packs its own inputs into page-locked
 * staging (two sets of max_batch requests per queue in use) and copies its own outputs back.  Status words go to their own caller
 * only; if a batched call fails as a whole (< 0), its requests are run again one by one, so every caller gets exactly what its
 * uncoalesced call returns.  max_batch = 0 switches it off.  The _batch and _dev entry points are never coalesced. */
int mp_set_coalesce(mp_table* t, size_t max_batch, uint32_t max_wait_us);
/* counters since the last mp_set_coalesce: out[0] requests served, [1] batched calls run, [2] largest batch, [3] batches closed full,
 * [4] batches closed by time, [5] requests re-run one by one after a failed batched call, [6] summed queue wait (arrival to the start
 * of its batched call) in microseconds, [7] reserved (0) */
int mp_coalesce_stats(const mp_table* t, uint64_t out[8]);

/* ---- batched forms: B independent proofs, arrays of the single-proof buffers back to back -------------------
 * status[b] receives the per-proof result; the return value is < 0 only for call-level errors. */
int mp_shuffle_and_remask_batch(mp_table* t, size_t B, const uint8_t* decks, const uint8_t* masking_factors,
                                const uint32_t* permutations, const uint8_t* prover_seeds, uint8_t* out_decks,
                                uint8_t* out_proofs, int32_t* status);
int mp_verify_shuffle_batch(mp_table* t, size_t B, const uint8_t* decks, const uint8_t* shuffled_decks,
                            const uint8_t* proofs, int32_t* status);

/* ---- device-resident forms: every pointer is a DEVICE pointer (HBM).  All kernels are enqueued on the context's stream
 * (mp_sync waits for them).  The prover returns without waiting.  The verifier waits ONCE inside the call when merged
 * verification is on (the default): after the screening pass it reads one 4-byte flag back to decide whether the per-equation
 * pass has to run (it does only if some proof failed), so the call returns when the screening kernels have finished;
 * with mp_set_merged_verify(t, 0) it does not wait either.  d_status is written by the stream in both cases: read it after
 * mp_sync.  These are what bench.py times (inputs already in HBM). */
int mp_shuffle_and_remask_batch_dev(mp_table* t, size_t B, const void* d_decks, const void* d_masking_factors,
                                    const void* d_permutations, const void* d_prover_seeds, void* d_out_decks,
                                    void* d_out_proofs, void* d_status);
int mp_verify_shuffle_batch_dev(mp_table* t, size_t B, const void* d_decks, const void* d_shuffled_decks,
                                const void* d_proofs, void* d_status);
/* ---- keyed batches: one aggregate public key PER PROOF ----------------------------------------------------------------
 * A card server runs many tables at once; the tables share the public parameters (one mp_table) and differ only in their
 * aggregate key, which the reference passes per call (`shared_key`, [REF mod.rs:380-386, 420-426]).  shared_keys /
 * d_keys: B wire points.  The key's terms become per-proof work: the verifier gains one variable-base term, the prover
 * builds the key's own window tables (2^(5w) pk, w < 51) for the N re-encryptions rho_i * pk -- about 9 % more work per
 * prove+verify than under the table's fixed key.  Results are byte-identical to a table created with that key. */
/* a table of the shared parameters alone (no aggregate key): accepts only the _keys entry points */
int mp_table_create_params(mp_ctx* ctx, uint32_t m, uint32_t n, const uint8_t* params, uint32_t fb_window_bits, mp_table** out);
int mp_shuffle_and_remask_batch_keys(mp_table* t, size_t B, const uint8_t* shared_keys, const uint8_t* decks,
                                     const uint8_t* masking_factors, const uint32_t* permutations, const uint8_t* prover_seeds,
                                     uint8_t* out_decks, uint8_t* out_proofs, int32_t* status);
int mp_verify_shuffle_batch_keys(mp_table* t, size_t B, const uint8_t* shared_keys, const uint8_t* decks,
                                 const uint8_t* shuffled_decks, const uint8_t* proofs, int32_t* status);
int mp_shuffle_and_remask_batch_keys_dev(mp_table* t, size_t B, const void* d_keys, const void* d_decks,
                                         const void* d_masking_factors, const void* d_permutations, const void* d_prover_seeds,
                                         void* d_out_decks, void* d_out_proofs, void* d_status);
int mp_verify_shuffle_batch_keys_dev(mp_table* t, size_t B, const void* d_keys, const void* d_decks, const void* d_shuffled_decks,
                                     const void* d_proofs, void* d_status);
/* ---- key sets: the aggregate keys of many card tables, prepared once ---------------------------------------------------------
 * A card table keeps its aggregate key for as long as its players stay [REF examples/round.rs:228-262: the key is computed once,
 * before the shuffles], so a server that runs many tables can hand their keys over ahead of time: mp_keyset_create builds
 * fixed-base window tables for every key (8-bit windows: 8 160 points = 0.5 MB per key on the 256-bit curves, in HBM) and the
 * _keyset entry points name a proof's key by its index in the set (d_key_index: B uint32, device memory).  The N
 * re-encryptions rho_i * pk then cost 32 table additions each and no per-proof table construction (keyed batches without a
 * set: 51 additions plus the key's own window tables per proof).  Results are byte-identical to the _keys entry points and to
 * a table created with that key.  keys: n_keys wire points in HOST memory; each must be a point of the prime-order group other
 * than the identity (MP_ERR_BAD_ENCODING otherwise).  An index >= n_keys gives status MP_ERR_BAD_ARGUMENT for that proof.
 * A key set belongs to the table it was created for and must be destroyed before it. */
typedef struct mp_keyset mp_keyset;
int mp_keyset_create(mp_table* t, size_t n_keys, const uint8_t* keys, mp_keyset** out);
void mp_keyset_destroy(mp_keyset* ks);
size_t mp_keyset_size(const mp_keyset* ks);
int mp_shuffle_and_remask_batch_keyset_dev(mp_table* t, const mp_keyset* ks, size_t B, const void* d_key_index, const void* d_decks,
                                           const void* d_masking_factors, const void* d_permutations, const void* d_prover_seeds,
                                           void* d_out_decks, void* d_out_proofs, void* d_status);
int mp_verify_shuffle_batch_keyset_dev(mp_table* t, const mp_keyset* ks, size_t B, const void* d_key_index, const void* d_decks,
                                       const void* d_shuffled_decks, const void* d_proofs, void* d_status);
/* ---- key sets whose slots change: one table of thousands reseats between two hands --------------------------------------------
 * A set is mp_keyset_size(ks) SLOTS, each live (it holds a key) or empty.  The set's device buffers are allocated once, for every
 * slot, when it is created, and never move.  mp_keyset_create makes a set of n_keys live slots; mp_keyset_create_empty one of
 * `capacity` empty slots (same limits).  mp_keyset_live: the number of live slots (takes the context's lock and waits for the
 * updates in flight).
 *
 * mp_keyset_update[_dev] puts keys[i] (wire points; the _dev form: device memory) into slot slots[i], i < count, and builds the window
 * tables of these `count` keys only, on the device, in slices of 1 024 keys whose staging the set keeps (a full slice:
 * about 1.6 GB on the 256-bit curves for an update of that size or more, less for a smaller one).  Every key is validated on the
 * device: canonical, on the curve, not the identity, in the prime-order subgroup -- whatever mp_set_subgroup_check says.
 *   status[i] == MP_OK                slot slots[i] is live with key i
 *   status[i] == MP_ERR_BAD_ENCODING  slot slots[i] is EMPTY, whatever it held before: a server that misses the word does not go on
 *                                     serving the departed players' key under the table's index.  The other slots of the call are
 *                                     not affected.
 * mp_keyset_clear empties the named slots.
 *
 * `slots` is a HOST array in every form (the rule of `first` and `links` of the ragged calls): it is copied and the copy is checked
 * before anything is enqueued.  count == 0, a slot >= mp_keyset_size(ks) or a slot named twice: the call returns MP_ERR_BAD_ARGUMENT,
 * nothing is enqueued, the set is unchanged and no buffer of the caller's is touched.
 *
 * Ordering.  An update is enqueued on the context's stream behind everything the context holds on both lanes; pipelined verify calls
 * whose screening verdicts are still unexamined (mp_set_pipeline) are completed first.  A call issued before the update sees the old
 * keys, a call issued after it the new ones.  mp_keyset_update and mp_keyset_clear return when done; mp_keyset_update_dev returns when
 * queued: d_keys must stay as it is, and d_status is final, after mp_sync.
 *
 * A proof that names an empty slot gets what an index >= mp_keyset_size(ks) gets: status MP_ERR_BAD_ARGUMENT for that proof, its
 * outputs computed under slot 0 as they are for such an index, the other proofs of the batch untouched.  No kernel reads outside
 * the set's buffers for any index. */
int mp_keyset_create_empty(mp_table* t, size_t capacity, mp_keyset** out);
size_t mp_keyset_live(const mp_keyset* ks);
int mp_keyset_update(mp_keyset* ks, size_t count, const uint32_t* slots, const uint8_t* keys, int32_t* status);
int mp_keyset_update_dev(mp_keyset* ks, size_t count, const uint32_t* slots, const void* d_keys, void* d_status);
int mp_keyset_clear(mp_keyset* ks, size_t count, const uint32_t* slots);
/* Keys by index where a round needs them.  Results are byte- and word-identical to the key-passing forms with the set's keys written out.
 *
 * mp_shuffle_and_remask_batch_seeded_keyset_dev is mp_shuffle_and_remask_batch_seeded_dev (below) with a set and one index per proof
 * (d_key_index: B uint32, device memory) in place of d_keys; the keys' multiples come from the set's tables, as in
 * mp_shuffle_and_remask_batch_keyset_dev.
 *
 * mp_verify_shuffle_chain_ragged_keyset[_dev] are mp_verify_shuffle_chain_ragged[_dev] (below) with ONE index per TABLE -- key_index: a
 * host array of `tables` uint32 in the host form, a device array in the _dev form -- instead of one key per link: the per-link keys the
 * chain verifier wants are written on the device.  A table whose index is >= mp_keyset_size(ks) or names an empty slot gets
 * MP_ERR_BAD_ARGUMENT on every one of its links; the other tables are unaffected.  Both piece modes apply (mp_set_chain_pieces).
 *
 * mp_mask_batch_keyset, mp_verify_mask_batch_keyset and mp_verify_mask_batch_keyset_dev are mp_mask_batch, mp_verify_mask_batch and
 * mp_verify_mask_batch_dev (below) with a set in place of `K` and `keys`: key_index[c] names a slot.  The prover takes its two products
 * with the key, r pk for the masked card and w pk for the commitment, from the set's tables -- at most 32 table additions each and no
 * window table of pk per card; the verifier reads the key from the set.  A card on an empty slot or past the set gets
 * MP_ERR_BAD_ARGUMENT (and zero bytes from the prover), as a key index past `K` does.  mp_set_sigma_screen applies as to
 * mp_verify_mask_batch.  A set's keys were tested for subgroup membership when they entered; the calls do not test them again.
 *
 * mp_keyset_seat_ragged_batch is mp_aggregate_keys_ragged_batch (below) whose sums go into the slots slots[k] of the set without leaving
 * the device, through the validation and the table build of mp_keyset_update: player_status, table_status and out_keys (which may be
 * NULL) are that call's words and bytes.  slot_status[k]: MP_OK, slot slots[k] is live under table k's aggregate key; table_status[k]
 * where that is not 0, or MP_ERR_BAD_ENCODING where every proof is good and the sum is the identity (keys pk and -pk): the slot is
 * EMPTY.  `slots` follows the rules of mp_keyset_update; uniform seating is first[k] = k * P. */
int mp_mask_batch_keyset(mp_table* t, const mp_keyset* ks, int kind, size_t C, const uint32_t* key_index, const uint8_t* inputs,
                         const uint8_t* factors, const uint8_t* prover_seeds, uint8_t* out_masked, uint8_t* out_proofs, int32_t* status);
int mp_verify_mask_batch_keyset(mp_table* t, const mp_keyset* ks, int kind, size_t C, const uint32_t* key_index, const uint8_t* inputs,
                                const uint8_t* masked, const uint8_t* proofs, int32_t* status);
int mp_verify_mask_batch_keyset_dev(mp_table* t, const mp_keyset* ks, int kind, size_t C, const void* d_key_index, const void* d_inputs,
                                    const void* d_masked, const void* d_proofs, void* d_status);
int mp_keyset_seat_ragged_batch(mp_keyset* ks, size_t tables, const uint32_t* first, const uint32_t* slots, const uint8_t* keys,
                                const uint8_t* proofs, const uint8_t* fs_init, uint8_t* out_keys, int32_t* player_status, int32_t* table_status,
                                int32_t* slot_status);
int mp_shuffle_and_remask_batch_seeded_keyset_dev(mp_table* t, const mp_keyset* ks, size_t B, const void* d_key_index, const void* d_decks,
                                                  const void* d_seeds, void* d_out_decks, void* d_out_proofs, void* d_status, void* d_out_perms,
                                                  void* d_out_factors);
int mp_verify_shuffle_chain_ragged_keyset(mp_table* t, const mp_keyset* ks, size_t tables, const uint32_t* links, const uint32_t* key_index,
                                          const uint8_t* decks, const uint8_t* proofs, int32_t* status);
int mp_verify_shuffle_chain_ragged_keyset_dev(mp_table* t, const mp_keyset* ks, size_t tables, const uint32_t* links, const void* d_key_index,
                                              const void* d_decks, const void* d_proofs, void* d_status);
/* ---- chain verification: the shuffle chain of a card table verified as one equation -------------------------------------------
 * A table's deck passes through `links` shuffles (deck_{j+1} = output of link j [REF examples/round.rs:268-350]) and every one of
 * them is verified.  These entry points verify `tables` chains at once; decks: (links + 1) x tables decks, deck j of table t at index
 * j * tables + t; proofs / status / keys: links x tables, link j of table t at j * tables + t (keys: the table's aggregate key repeated
 * per link; NULL = the mp_table's own key).  The merged equations of a chain's links are added up with weights that depend on every
 * proof of the chain, so every inner deck is a base once instead of twice and the n + 5 fixed bases appear once per table; the MSM runs on
 * the bucket kernel.  A table whose chain fails is re-verified link by link: status words are identical to mp_verify_shuffle_batch*. */
int mp_verify_shuffle_chain(mp_table* t, size_t tables, uint32_t links, const uint8_t* shared_keys, const uint8_t* decks,
                            const uint8_t* proofs, int32_t* status);
int mp_verify_shuffle_chain_dev(mp_table* t, size_t tables, uint32_t links, const void* d_keys, const void* d_decks, const void* d_proofs,
                                void* d_status);
/* mp_verify_shuffle_chain_ragged[_dev]: the tables of one call may have chains of different lengths, links[t] >= 1 links for table t.
 * The layout is table-major -- link-major needs equal lengths: with off(t) = links[0] + ... + links[t-1], table t owns
 * the decks off(t) + t .. off(t) + t + links[t] (consecutive: deck j + 1 is the output of link j) and the proofs, status words and keys
 * off(t) .. off(t) + links[t] - 1 (keys: one per link; NULL = the mp_table's own key).
 *
 * Pieces and passes.  The chain of table t is cut into PIECES (t, first link a, length l) -- the links a .. a + l - 1 and their l + 1
 * decks --, and the pieces of one length l, in (t, a) order, are a PASS: gathered ON THE DEVICE into link-major staging (one launch per
 * pass, kernels_chain_pieces.hpp) and verified by one mp_verify_shuffle_chain_dev call of (pieces of the pass) tables x l links.
 * mp_set_chain_group, _max_links and _slice apply to each pass as to a call of that pass alone.  Once every pass has been enqueued, ONE
 * launch scatters the words of all passes into the status array: on a return other than MP_OK the status array is as it was.  The
 * status words are those of mp_verify_shuffle_batch[_keys] link by link, whatever the decomposition (mp_set_chain_pieces):
 *   MP_CHAIN_PIECES_WHOLE   one piece per table; the passes are the distinct values of links[t], ascending.  Every inner deck of a chain
 *                           is a base of its equation once.
 *   MP_CHAIN_PIECES_BINARY  the chain is cut front to back into pieces whose lengths are the powers of two in links[t], largest first
 *                           (7 = 4 + 2 + 1); the passes are the distinct piece lengths, ascending: at most 12 whatever the lengths, 4 for
 *                           2 to 10 links, each of them wide.  A deck at a cut is a base of two equations.  The cut is made only
 *                           where it saves passes: a call in which whole chains need no more passes than their pieces -- every call
 *                           whose chains have one length -- is verified as under MP_CHAIN_PIECES_WHOLE.
 * tables == 0, a links[t] of 0 or above 4 095, 2^31 proofs and more, a keyless table without keys: MP_ERR_BAD_ARGUMENT, nothing is
 * enqueued and no buffer is touched.
 *
 * _dev: d_keys (or NULL), d_decks, d_proofs and d_status are device arrays in the layout above, 16-byte aligned; `links` is ALWAYS a host
 * array, with the rules of `first` of the other ragged _dev calls: it is copied and the copy is validated before anything is enqueued,
 * only the copy is used, and the caller's array is consumed when the call returns.  d_status is final after mp_sync.
 * The host-buffer form uploads the caller's arrays as they are, once, takes the _dev path and downloads the words, once: the library
 * copies no deck, proof or key within host memory.
 *
 * Staging.  The table keeps the staging of a pass, the words of all passes and the descriptors; they grow only, a call that fits what is
 * there allocates nothing, and they go with mp_table_destroy.  With P passes of G_p pieces of l_p links, deck_bytes = 2 m n point_bytes:
 *   max_p (l_p + 1) G_p * deck_bytes  +  max_p l_p G_p * (proof_bytes + point_bytes if keys are passed)
 *   + 4 * sum(links)  +  16 * pieces  +  24 * P      bytes
 * (the host-buffer form keeps device copies of its three arrays and of the status words on top). */
#define MP_CHAIN_PIECES_WHOLE 0
#define MP_CHAIN_PIECES_BINARY 1
int mp_verify_shuffle_chain_ragged(mp_table* t, size_t tables, const uint32_t* links, const uint8_t* shared_keys, const uint8_t* decks,
                                   const uint8_t* proofs, int32_t* status);
int mp_verify_shuffle_chain_ragged_dev(mp_table* t, size_t tables, const uint32_t* links, const void* d_keys, const void* d_decks,
                                       const void* d_proofs, void* d_status);
/* How mp_verify_shuffle_chain_ragged[_dev] cuts its chains: MP_CHAIN_PIECES_WHOLE or MP_CHAIN_PIECES_BINARY (anything else:
 * MP_ERR_BAD_ARGUMENT).  Status words do not depend on it. */
int mp_set_chain_pieces(mp_table* t, int mode);
/* The last mp_verify_shuffle_chain_ragged[_dev] call on this table that passed its argument checks: out[0] passes, [1] pieces, [2] tables,
 * [3] links, [4] bytes moved by the gather launches, [5] bytes of decks, proofs and keys the library copied within host memory -- the constant
 * 0, not a counter: the call has no such copy, and the word keeps its place for callers that budgeted the host staging of the earlier
 * implementation --, [6] pieces of the widest pass, [7] the cut that was made (MP_CHAIN_PIECES_WHOLE also where the table is set to
 * MP_CHAIN_PIECES_BINARY and the cut would have saved no pass).  Takes the context's lock. */
int mp_chain_ragged_stats(const mp_table* t, uint64_t out[8]);
int mp_sync(mp_ctx* ctx);
int mp_reserve(mp_table* t, size_t B);           /* pre-allocate the batch workspace for B proofs */
/* Every table holds six static work splits with identical results: a throughput plan (large sub-jobs, fewest operations) and five
 * finer ones -- wide, medium, latency, small, finest -- that give a proof more lanes (smaller sub-jobs; the windows of a variable-base
 * sub-job dealt to several lanes).  Batches of at most B / 20 proofs use the finest split, up to 0.3 B the small one, up to `B` the
 * latency plan, up to 2.4 B the medium plan, up to 19.2 B the wide plan, larger ones the throughput plan (default B = 2560 * 52 / N, at
 * least 40: 128 / 768 / 2 560 / 6 144 / 49 152 proofs of 52 cards, the crossovers measured on an MI355X; 0 = always throughput). */
int mp_set_latency_batch(mp_table* t, size_t B);
/* Every batch takes work split `split` whatever its size: 0 throughput, 1 latency, 2 medium, 3 finest, 4 wide, 5 small; -1 (default) =
 * by batch size as above.  For tests and measurements: the results do not depend on it. */
int mp_set_work_split(mp_table* t, int split);
/* Pipelined verification (depth 0 = off, the default).  A card server proves the next batch while the previous one is verified;
 * with depth >= 1 the device-resident verify calls (mp_verify_shuffle_batch[_keys|_keyset]_dev) run on a second lane of the context --
 * streams and arenas of their own -- ordered behind everything the context held when they were issued, and return WITHOUT waiting for
 * their screening verdict, so that the caller's next mp_shuffle_and_remask_batch*_dev call runs beside them on the chip (batches that
 * do not fill it alone).  The verdict of verify call k is looked at when verify call k + depth comes in, or at
 * mp_sync; only then -- and only if some proof failed the screen -- does the per-equation pass of call k run.  The caller's side of
 * the contract: the buffers a verify call reads (decks, shuffled decks, proofs, keys) stay untouched until `depth` further verify
 * calls on that table, or mp_sync, have returned (rotate depth + 1 sets of prover outputs); d_status is final after mp_sync, as
 * before.  Status words are identical in every mode.  The host-buffer entry points and chain verification are unaffected.
 * (A context owns four HIP streams -- two lanes of two -- which the runtime's default of four hardware queues serves.) */
int mp_set_pipeline(mp_table* t, int depth);
/* The sizes behind work split `split` (0 .. 5 as above): fixed-base / variable-base terms per sub-job, bases per window-table lane,
 * points per shared inversion, and `window_lanes` = lanes per variable-base sub-job: the Straus windows of a sub-job are dealt to that
 * many lanes (each runs its share as a chain of its own) and one fold per multi-scalar multiplication puts the range sums together --
 * k times the lanes for < 250 extra doublings per MSM instead of k times the doubling chains (1 = one lane runs all windows).
 * mp_set_plan_thresholds: the largest batch that takes the finest / small / latency / medium / wide split.  For measurements and tuning on
 * other parts: results do not depend on either.  Both rebuild nothing a running batch uses (call between batches). */
int mp_set_plan_params(mp_table* t, int split, uint32_t fixed_terms, uint32_t var_terms, uint32_t table_group, uint32_t norm_chunk,
                       uint32_t window_lanes);
int mp_set_plan_thresholds(mp_table* t, size_t finest, size_t small, size_t latency, size_t medium, size_t wide);
/* Verification strategy.  on (default): the verifier first evaluates ALL group equations of a proof merged into one
 * multi-scalar multiplication with random weights derived from the whole proof (soundness loss ~2^-250); a batch in which
 * every proof passes ends there.  The proofs that fail it -- they and nobody else (round 5, mp_set_group_refine below) -- are evaluated
 * equation by equation, so that the FIRST failing check is reported by name exactly as the reference does [REF tests.rs:223-225].
 * off: always evaluate the equations one by one.  Results (status words) are identical in both modes. */
int mp_set_merged_verify(mp_table* t, int on);
/* Group verification (round 4; on by default).  The screening pass of a batch of at least `min_batch` x 52 / N proofs (default 6 144 for
 * 52-card decks) adds the merged equations of a GROUP of proofs with weights derived from every proof of the group and evaluates the
 * sum as ONE multi-scalar multiplication by the bucket method: 18 to 32 additions per point instead of 51 plus window tables and
 * doubling chains, and the fixed bases once per group.  Round 6: from 8/3 `min_batch` (16 384) proofs on, the equations hold up to
 * `points_per_group` points (default 243 712: a proof brings 4N + 11m + 8, so 1 024 proofs of a 52-card deck, 64 of a 1 024-card one)
 * and run on the split pipeline (mp_set_bucket_split: 14-bit windows, 18 additions per point) as long as min_batch / 512 (12)
 * equations of at least 50 000 points are left; smaller batches take the rule of rounds 4-5 -- at most 30 464 points (128 proofs) and no
 * fewer than 2/13 `min_batch` (945) groups: 8 proofs per group at 8 192 in flight, one wave per window.  points_per_group <= 65 535
 * asks for that rule at every batch size (30 464 = the default of rounds 4-5).  The group size is the divisor of the batch size nearest
 * to the target (between half and twice it; a batch without one keeps the per-proof screen).  BLS12-377: the split pipeline only (its
 * hot loop is spill-free on the 14-limb field; equations from 40 000 points on, 11-bit windows included).  A group whose equation
 * fails is looked at more closely -- ITS members only (below): status words are identical to every other strategy.  points_per_group
 * = 0 switches it off.  Needs merged verification on.  mp_group_size: the group size a batch of B proofs takes under the table's own
 * key (0: per-proof screen).  (52-card decks at 262 144 in flight: 524 k proofs/s without groups, 672 k with the groups of round 5,
 * 717 k with those of round 6 on the same kind of box.) */
int mp_set_group_verify(mp_table* t, uint32_t points_per_group, size_t min_batch);
uint32_t mp_group_size(const mp_table* t, size_t B);
/* What a rejected proof costs (round 5).  A screen that fails -- the merged equation of one proof, the equation of a group of proofs,
 * of a chain -- names the proofs it could not clear; only THEY are looked at again: their inputs are gathered into a contiguous
 * sub-batch on the device, the sub-batch takes the next finer pass and its status words are written back over the screen's marks.
 * Everybody else's verdict stands, as in the reference, where one call verifies one proof [REF src/discrete_log_cards/mod.rs:420-443].
 * The members of failing groups go through equations of sub-groups of `points_per_subgroup` points (0 = default: an eighth of the group
 * equation's -- 128 proofs of a 52-card deck under an equation of 1 024, and an eighth of THAT, 16, for the members of failing
 * sub-groups; a sixty-fourth at once when nearly every group of the call failed) when there are at least `min_subgroups` of them (0 =
 * default 128: enough to fill the bucket kernel), otherwise -- and after two such levels always -- through the per-equation pass that
 * names the first failing check.  One tampered proof among 262 144 sends the 1 024 members of its equation through that pass: +2.7 ms
 * on a 90 ms verify call.  The suspects are gathered and looked at in slices of at most 131 072 52-card proofs (bounded memory whatever
 * their number), and until a suspect has its own word its status reads MP_ERR_INTERNAL, never 0.  mp_reverified_count: proofs that
 * have taken a per-equation pass on this table because a screen could not clear them. */
int mp_set_group_refine(mp_table* t, uint32_t points_per_subgroup, uint32_t min_subgroups);
uint64_t mp_reverified_count(const mp_table* t);
/* Groups that adapt to the rejection rate (default on).  A group fails if any member does, so with a fraction p of bad proofs in the traffic
 * 1 - (1 - p)^L of the groups of L fail (72 % of the groups of 128 at p = 1 %) and their members pay a finer pass on top of a screen that
 * cleared nobody.  The table remembers the last screens: when more than a fifth of a call's groups fail the next call takes groups of half
 * the size (down to 8; by three halvings at once when nineteen groups in twenty fail), when fewer than 4 % fail the size goes back up,
 * one step per call, two when no group failed (calls with at least 8 groups count, a step down needs four failing groups).  Honest
 * traffic never leaves the default size; verdicts do not depend on it.  on = 0 pins the default (and resets the memory); mp_group_size
 * reports the size the NEXT call of B proofs takes. */
int mp_set_group_adapt(mp_table* t, int on);
/* Variable-base MSMs with at least `terms` terms (default 2048: the verifier's products over a 1024-card deck) run on the
 * wave-cooperative bucket-method kernel (counting sort by wavefront prefix sum, balanced bucket shares, wave-wide bucket reduction),
 * smaller ones on the Straus kernel with per-proof window tables; 0 = never.  Results are identical; the split is a property of
 * the table's static plans, which this call rebuilds. */
int mp_set_bucket_min(mp_table* t, size_t terms);
/* Window width of the bucket method: 8 to 14 bits (128 to 8 192 buckets per window; 32, 28, 26, 23, 21, 20 or 18 windows per 252-bit
 * scalar -- the smaller of k and q - k is recoded, signs flipped: ceil(bits / c) windows), or 0 (default) = by the size of the MSM (8
 * bits below 6 000 terms, 9 below 12 000, 10 below 40 000, 11 below 50 000, 12 below 200 000, 14 from there on -- the equation of a
 * group of 1 024 52-card proofs, mp_set_group_verify).  Results are identical; rebuilds the static plans like mp_set_bucket_min. */
int mp_set_bucket_bits(mp_table* t, uint32_t bits);
/* Round 6: inputs the caller has validated ONCE are not validated again in every call that touches them.  The reference's trait takes
 * typed arkworks points, validated when they were deserialised [REF examples/parameter_selection.rs:78-91]; this engine takes wire
 * bytes and by default tests every point of every call for membership of the prime-order subgroup (curves with a cofactor: BLS12-377)
 * -- a deck that passes along a chain of shuffles was tested in the call that proved it, the call that verified it and the call that
 * shuffled it on.  `what` = OR of MP_VALIDATED_*: the table's following calls skip the subgroup test of those inputs (range, curve
 * equation and permutation checks stay).  A deck is "validated" if it came out of mp_deck_deserialize_dev / mp_deck_deserialize with
 * status 0, out of mp_deck_validate_dev with status 0, or out of this engine's own prover.  0 (default) = test everything. */
#define MP_VALIDATED_DECKS 1u     /* the input decks of prove and verify calls */
#define MP_VALIDATED_SHUFFLED 2u  /* the shuffled decks of verify calls */
#define MP_VALIDATED_PROOFS 4u    /* the points of the proofs (only if they came through mp_proof_deserialize, or through
                                   * mp_proof_deserialize_dev / mp_proofs_deserialize_batch with status 0) */
int mp_set_validated(mp_table* t, uint32_t what);
/* `decks` wire-v1 decks of the table's size in DEVICE memory -> one int32 per deck in d_status: 0, or MP_ERR_BAD_ENCODING if a point is
 * not canonical, not on the curve or outside the prime-order subgroup.  The once-per-deck validation that mp_set_validated relies on. */
int mp_deck_validate_dev(mp_table* t, size_t decks, const void* d_wire_decks, void* d_status);
/* Round 6.  Bucket jobs whose windows are at least `min_bits` wide (default 12: equations of 50 000 points and more; 11 on BLS12-377)
 * run as a pipeline of kernels instead of one wave per (equation, window): k_bucket_sort (a workgroup per 24 576 terms: counting sort
 * inside LDS, the sorted run written in whole lines), k_bucket_acc (a wave per range of 256 buckets, four per lane dealt by rank, one
 * mixed addition per term; k_bucket_list -- equal shares of the sorted list -- where a window's digits crowd into a few buckets),
 * k_bucket_reduce (four waves per window, a quarter of the buckets each) and k_bucket_final.  10 .. 15 (= none).  Results are identical. */
int mp_set_bucket_split(mp_table* t, uint32_t min_bits);
/* Chain verification (mp_verify_shuffle_chain*): at most `links` links share one chain equation; longer chains are verified as
 * consecutive sub-chains.  0 (default) = as many as fit the 32 767 points of one equation (293 links of a 52-card deck; one link of a deck too large for that gets an equation of up to 65 535 points).  A smaller
 * value bounds the work that is repeated link by link when a chain fails.  Verdicts are the same. */
int mp_set_chain_max_links(mp_table* t, uint32_t links);
/* Chain verification of many tables at once: the chain equations of `tables_per_equation` tables are added up (with weights that
 * depend on every proof of every member, as in mp_set_group_verify) into ONE equation -- 64 tables x 4 392 points for 32 links of a
 * 52-card deck (round 6; 8 tables in round 5): 14-bit windows on the split pipeline, the points of an equation copied once into a
 * contiguous run (k_chain_tile), the fixed bases once per 64 tables.  0 (default) = by size: the divisor of `tables` that brings the
 * equation nearest to the group equation's points (mp_set_group_verify, under the same rule of how many equations must be left); 1 =
 * every table on its own (rounds 2-4); other values (up to 4 094, tables x (links + 1) <= 4 094) = the divisor of `tables` nearest to
 * it, whatever mp_set_group_verify says.  Tables g (tables / G) + e, g < G, share equation e.  If an equation fails, the links of ITS
 * tables are re-verified one by one: status words are identical in every setting. */
int mp_set_chain_group(mp_table* t, uint32_t tables_per_equation);
/* Chain verification in passes of `tables_per_pass` tables.  The workspace of chain verification is ~68 KB per link in flight (52-card
 * decks: 107 GB for 49 152 tables x 32 links), far more than the 13 KB of deck and proof a link occupies, while the prover wants as many
 * tables per call as there are (link j of every table is one batch).  0 (default) = one pass if the workspace fits the free device
 * memory, equal passes of whole thousands of tables otherwise; the rows of a pass are gathered from the link-major arrays on the device
 * (one copy per link and array).  Verdicts do not depend on it. */
int mp_set_chain_slice(mp_table* t, size_t tables_per_pass);
/* What a chain call does under the current settings: tables per equation for a pass of `tables` tables x `links` links (1 = every table
 * on its own), and the tables per pass the last mp_verify_shuffle_chain[_dev] call on this table took (0 = none yet). */
uint32_t mp_chain_group_size(const mp_table* t, size_t tables, uint32_t links, int keyed);
size_t mp_chain_last_slice(const mp_table* t);
/* Lanes per Fiat-Shamir transcript.  A proof's transcript is one BLAKE2s chain (13.6 KB of statement for a 52-card deck): 1 = one
 * lane per proof (what a batch that fills the chip wants), 4 = the four G functions of a half-round on four adjacent lanes (2.7x
 * fewer instructions in the chain: what a single proof or a few thousand large decks wait for), 0 (default) = 4 for batches of up
 * to 32 768 proofs, 1 above.  Digests, challenges and proofs are the same. */
int mp_set_transcript_lanes(mp_table* t, uint32_t lanes);
/* Lanes per group operation in the dependency chains of the multi-scalar multiplications (the Straus accumulators, the window fold
 * of the bucket method).  1 = one lane per chain (fewest instructions: what a batch that fills the chip wants); 4 = the independent
 * field products of a doubling / addition on four adjacent lanes, 3-4 products deep instead of 10-14 (what a single proof waits for:
 * every MSM has ~250 dependent doublings); 0 (default) = 4 while the chains of a launch need at most 65 536 lanes that way (a few
 * dozen 52-card proofs), 1 above.  The results are the same group elements. */
int mp_set_group_lanes(mp_table* t, uint32_t lanes);
/* How the prover evaluates the multi-exponentiation diagonals E_k (a polynomial product of the scalar rows with the ciphertext
 * rows) for 3 <= m <= 16.  on (default): Toom-Cook with the 2m points 0, inf, +-1 .. +-(m-1) -- 2m row products; off: recursive
 * Karatsuba (13 products at m = 4, 35 at m = 8; what m > 16 always uses).  m = 2 always uses its 4-point Toom-Cook form.  The
 * E_k are the same group elements either way: proof bytes do not change.  Rebuilds the table's static plans. */
int mp_set_toom_cook(mp_table* t, int on);
/* Curves with a cofactor (MP_CURVE_BLS12_377): every wire point of a call -- decks, keys, proof elements -- is tested for
 * membership in the prime-order subgroup ([q]P == O), as ark-ec's validating deserialiser does (the sigma calls included); failures give
 * MP_ERR_BAD_ENCODING for that proof.  on by default; a caller whose points were already validated (e.g. deserialised by
 * arkworks with checks) may switch it off -- it costs about three verifications per proof.  No effect on prime-order curves. */
int mp_set_subgroup_check(mp_table* t, int on);

/* ---- device pool: several contexts -- lanes of one GPU, or several GPUs -- behind one handle -----------------------------------------
 * The per-player proofs of a round are independent [REF examples/round.rs:263-350] and deterministic in their seeds, and contexts share
 * nothing, so a batch can be cut into contiguous blocks that run on several contexts at once.  A pool is `n_members` members; a member is
 * one mp_ctx on one device plus one persistent worker thread.  devices[i] is the device of member i; a device may appear several times --
 * those members are lanes that run side by side on that chip (batches that do not fill it alone) --, members on different devices are the
 * multi-GPU case; devices == NULL: member i runs on device i.  mp_ctx_create is the one-member case and stays what a caller with one
 * context per process uses.  n_members of 0 or above 64: MP_ERR_BAD_ARGUMENT; a device index that does not exist: MP_ERR_NO_DEVICE; either
 * way nothing is left allocated and mp_last_error names the member.  mp_pool_member_ctx: the context of member i, borrowed (NULL if there is
 * none): never to mp_ctx_destroy.  mp_pool_destroy: after every pool table of the pool has been destroyed and no call is in flight.
 * mp_pool_table_create: one mp_table per member from the one host copy of the parameters (shared_key NULL: keyless tables, as
 * mp_table_create_params).  The first member of every distinct device builds the fixed-base window tables -- the devices build at once,
 * each on its member's worker; tables are recomputed per GPU, nothing is copied between devices --, the further
 * members of that device build nothing and hold no second copy: they read the first member's tables (27-48 GB per table at the widest
 * windows).  fb_window_bits as mp_table_create_ex; 0 chooses the width once per device.  A build that fails on any member fails the call
 * with that member's code (the lowest member's, if several), mp_last_error names it, and the other members' tables are released.
 * mp_pool_table_member: the table of member i, BORROWED: valid until mp_pool_table_destroy, never to be passed to mp_table_destroy.  Settings
 * (mp_set_group_verify, mp_set_validated, mp_set_io_chunk, ...) are made per member through it -- the pool has no setter of its own but
 * mp_pool_set_min_shard --, and a device-resident caller shards its own batches over the members with the _dev entry points.
 * mp_pool_shuffle_and_remask_batch / mp_pool_verify_shuffle_batch: host buffers in the layout of mp_*_batch_keys; shared_keys NULL = the
 * table's own key (mp_*_batch).  The proofs [0, B) are cut into K contiguous blocks -- base, rem = divmod(B, K), the first rem blocks hold
 * one more -- for the first K = min(members, max(1, B / min_shard)) members (mp_pool_set_min_shard: proofs a block must hold before the call
 * takes another member, default 1); every worker runs the single-table call on its slice of every buffer and the caller's thread waits for
 * all of them.  Outputs and status[b] are byte for byte those of the same call on one mp_table.  Invalid arguments (null pointers, a keyless
 * table without shared_keys, B = 0) give the single-table call's return value, before anything is dispatched.  If a member's call fails as a
 * whole (< 0) the pool call returns the code of the lowest such member and mp_last_error, on the calling thread, its text behind "member i
 * (device d): "; the other members' blocks are complete.
 * Threads: pool calls from several host threads are safe and run one after the other (the pool's lock; the stats getters take it too);
 * calls made meanwhile on a borrowed member table from another thread are safe as well and take their turn through that context's lock.
 * mp_pool_stats: out[0] pool calls, [1] proofs, [2] members the last call used, [3] fixed-base table builds performed (= distinct devices),
 * [4] members, [5..7] reserved (0).  mp_pool_member_stats: out[0] device, [1] calls that gave member i a block, [2] its proofs, [3] its busy
 * time in microseconds (host clock around the member's calls).
 * Not offered through the pool: chain verification (its link-major layout needs a strided gather), the seeded prover, the sigma, deal and
 * open calls, device-resident pool calls (shard over mp_pool_table_member), and any collective: the library does not use RCCL. */
typedef struct mp_pool mp_pool;
typedef struct mp_pool_table mp_pool_table;
int mp_pool_create(int curve_id, size_t n_members, const int* devices, mp_pool** out);
void mp_pool_destroy(mp_pool* p);
size_t mp_pool_size(const mp_pool* p);
mp_ctx* mp_pool_member_ctx(mp_pool* p, size_t i);
int mp_pool_table_create(mp_pool* p, uint32_t m, uint32_t n, const uint8_t* params, const uint8_t* shared_key, uint32_t fb_window_bits,
                         mp_pool_table** out);
void mp_pool_table_destroy(mp_pool_table* pt);
mp_table* mp_pool_table_member(mp_pool_table* pt, size_t i);
int mp_pool_set_min_shard(mp_pool_table* pt, size_t proofs);
int mp_pool_shuffle_and_remask_batch(mp_pool_table* pt, size_t B, const uint8_t* shared_keys, const uint8_t* decks,
                                     const uint8_t* masking_factors, const uint32_t* permutations, const uint8_t* prover_seeds,
                                     uint8_t* out_decks, uint8_t* out_proofs, int32_t* status);
int mp_pool_verify_shuffle_batch(mp_pool_table* pt, size_t B, const uint8_t* shared_keys, const uint8_t* decks, const uint8_t* shuffled_decks,
                                 const uint8_t* proofs, int32_t* status);
int mp_pool_stats(const mp_pool_table* pt, uint64_t out[8]);
int mp_pool_member_stats(const mp_pool_table* pt, size_t i, uint64_t out[4]);

/* ---- building blocks (host buffers) ------------------------------------------------------------------------
 * mp_remask_batch: out[i] = in[i] + (rho_i * G, rho_i * pk)        [REF remasking.rs:16-18]
 * mp_msm:          n_msm independent variable-base MSMs of k terms: out[j] = sum_t scalars[j][t] * points[j][t]
 * mp_commit_batch: Pedersen com(v; r) = r*H + sum v_l * ck_l, `count` commitments of `len` <= n values each */
int mp_remask_batch(mp_table* t, size_t count, const uint8_t* cards, const uint8_t* masking_factors, uint8_t* out);
int mp_msm(mp_table* t, size_t n_msm, size_t k, const uint8_t* scalars, const uint8_t* points, uint8_t* out);
int mp_commit_batch(mp_table* t, size_t count, size_t len, const uint8_t* values, const uint8_t* r, uint8_t* out);

/* ---- sigma protocols behind the rest of DLCards (host buffers) -------------------------------------
 * nbases = 1: Schnorr identification (prove/verify_key_ownership, [REF mod.rs:132-165]);
 * nbases = 2: Chaum-Pedersen DL equality (mask / remask / reveal proofs and their verifiers, [REF mod.rs:182-357]).
 * Per proof: bases g_i, publics a_i = x * g_i (nbases points each), witness x, `fs_init` = Blake2s digest of the bytes the
 * reference seeds its FiatShamirRng with (mp_blake2s of e.g. b"Masking Proof"), prover seed; proof = A_1..A_nb || z.
 * verify status: 0 Ok, 5 "Schnorr Identification", 6 "Chaum-Pedersen" [REF tests.rs:74-76,120,170], < 0 usage error.
 * Wire points are validated like those of the shuffle calls: a base, a public or (verify) a commitment that is not canonical, not
 * on the curve or -- on a curve with a cofactor, subject to mp_set_subgroup_check -- outside the prime-order subgroup gives
 * MP_ERR_BAD_ENCODING for that proof, on the prover's side too (z g - c a - A = O also holds for a + L whenever c L = O, so without
 * the test a key or a reveal token shifted by a low-order point L would be accepted with probability 1 / ord(L)).  A witness or a
 * response >= q is MP_ERR_BAD_ENCODING as well.
 * The nonce is hedged ("sigma transcript v2"): r = Fr::rand(ChaCha20Rng(Blake2s(ToBytes(bases, publics) || Blake2s(witness || fs_init ||
 * prover_seed)))), so a repeated seed repeats the nonce only if witness and statement repeat too (the reference's `rng: &mut R` advances
 * by itself; an explicit seed does not).  Seeds should still be fresh CSPRNG output per call (`rng.fill_bytes`). */
int mp_sigma_prove_batch(mp_table* t, size_t B, uint32_t nbases, const uint8_t* bases, const uint8_t* publics,
                         const uint8_t* witness, const uint8_t* fs_init, const uint8_t* prover_seeds, uint8_t* out_proofs,
                         int32_t* status);
int mp_sigma_verify_batch(mp_table* t, size_t B, uint32_t nbases, const uint8_t* bases, const uint8_t* publics,
                          const uint8_t* proofs, const uint8_t* fs_init, int32_t* status);
int mp_blake2s(const uint8_t* in, size_t len, uint8_t out[32]);   /* host helper: BLAKE2s-256 */

/* ---- opening cards in batches: reveal tokens with their proofs, and unmasking [REF mod.rs:300-378; examples/round.rs:159-206, 352-430]
 * After the shuffles every card that is looked at or shown takes one reveal token with a Chaum-Pedersen proof from each player, and
 * whoever opens the card verifies the proofs and computes c1 - sum of the tokens.  One call carries the cards of many tables:
 *   keys     K wire points: the players' public keys of all tables of the call        cards    C masked cards (c0 || c1)
 *   T        tokens per card                                                          signer   C x T uint32: signer[c T + j] = index into
 *   keys of the player whose token j of card c is; everything per token is in the lane order c T + j.
 * mp_reveal_batch (a player): token = secret_keys[signer] * c0 with the "sigma transcript v2" proof for the bases (c0, G), the publics
 * (token, keys[signer]) and fs_init = Blake2s("Reveal Proof") -- the bytes of mp_msm followed by mp_sigma_prove_batch on those inputs, one
 * window table of c0 for token and commitment.  secret_keys: K scalars in the order of keys (pk = sk * G is NOT checked, as in the
 * reference: such a proof does not verify); prover_seeds: C x T x 32 fresh random bytes; status[c T + j]: 0 or < 0.
 * mp_unmask_batch (whoever opens): token_status[c T + j] = 0, 6 "Chaum-Pedersen", MP_ERR_BAD_ENCODING (token, key, card point or
 * commitment not canonical, not on the curve or -- subject to mp_set_subgroup_check -- outside the prime-order subgroup; response >= q)
 * or MP_ERR_BAD_ARGUMENT (signer >= K); card_status[c] = the first token_status of the card that is not 0, in j order (the reference
 * fails at the first bad token).  A card with status 0: out_plain[c] = c1 - sum_j token as a canonical wire point and out_index[c] = the
 * smallest i with plain_cards[i] == out_plain[c] as bytes, or 0xFFFFFFFF; any other card: zero bytes and 0xFFFFFFFF.  The tokens of a
 * card are summed as given: that they come from distinct players, or from all of them, is the caller's to check, as in the reference.
 * plain_cards: n_plain <= 4 096 wire points (NULL if 0), validated once per call as encodings: a bad one is MP_ERR_BAD_ENCODING for the call.
 * Limits: 1 <= T, C * T <= 1 048 576, 1 <= K <= 1 048 576 (MP_ERR_BAD_ARGUMENT otherwise).  Keyed and keyless tables alike (of the
 * parameters only G is used); never coalesced.
 * mp_unmask_batch_dev: the same with every pointer a DEVICE pointer -- d_cards may be the d_out_decks of the prover -- enqueued on the
 * context's stream; the outputs are final after mp_sync.  (With n_plain > 0 the call waits once for the stream and reads the card list
 * back to validate it.)  The buffers stay untouched until then. */
int mp_reveal_batch(mp_table* t, size_t K, const uint8_t* keys, const uint8_t* secret_keys, size_t C, const uint8_t* cards, uint32_t T,
                    const uint32_t* signer, const uint8_t* prover_seeds, uint8_t* out_tokens, uint8_t* out_proofs, int32_t* status);
int mp_unmask_batch(mp_table* t, size_t K, const uint8_t* keys, size_t C, const uint8_t* cards, uint32_t T, const uint32_t* signer,
                    const uint8_t* tokens, const uint8_t* proofs, size_t n_plain, const uint8_t* plain_cards, uint8_t* out_plain,
                    uint32_t* out_index, int32_t* token_status, int32_t* card_status);
int mp_unmask_batch_dev(mp_table* t, size_t K, const void* d_keys, size_t C, const void* d_cards, uint32_t T, const void* d_signer,
                        const void* d_tokens, const void* d_proofs, size_t n_plain, const void* d_plain_cards, void* d_out_plain,
                        void* d_out_index, void* d_token_status, void* d_card_status);
/* The same three calls for cards with DIFFERENT numbers of tokens (tables of 2 to 10 seats in one call): instead of T an offsets array
 *   first    C + 1 uint32: card c owns the lanes first[c] .. first[c+1] - 1; first[0] == 0, strictly increasing (every card has at
 *   least one token), first[C] <= 1 048 576 = the number of lanes of the call.
 * Everything per token -- signer, tokens, proofs, prover_seeds, status words -- comes in lane order.  `first` is ALWAYS a host array, in
 * the _dev form too: the library copies it, validates the copy on the host and uploads THAT into a buffer the table keeps, so a
 * malformed array is MP_ERR_BAD_ARGUMENT for the call with nothing enqueued and no buffer touched, never an index out of range on the
 * device; the caller's array -- pageable or page-locked -- is consumed before the call returns.  Everything else is what the uniform calls promise, per card: the status words, zero bytes for
 * lanes and cards that fail, card_status[c] = the first token status of the card that is not 0 in lane order, out_index, the validation of
 * the card list, the subgroup checks, mp_set_sigma_screen, the other limits; never coalesced.  With first[c] = c * T the outputs are
 * the bytes and words of the uniform call. */
int mp_reveal_ragged_batch(mp_table* t, size_t K, const uint8_t* keys, const uint8_t* secret_keys, size_t C, const uint8_t* cards,
                           const uint32_t* first, const uint32_t* signer, const uint8_t* prover_seeds, uint8_t* out_tokens,
                           uint8_t* out_proofs, int32_t* status);
int mp_unmask_ragged_batch(mp_table* t, size_t K, const uint8_t* keys, size_t C, const uint8_t* cards, const uint32_t* first,
                           const uint32_t* signer, const uint8_t* tokens, const uint8_t* proofs, size_t n_plain, const uint8_t* plain_cards,
                           uint8_t* out_plain, uint32_t* out_index, int32_t* token_status, int32_t* card_status);
int mp_unmask_ragged_batch_dev(mp_table* t, size_t K, const void* d_keys, size_t C, const void* d_cards, const uint32_t* first,
                               const void* d_signer, const void* d_tokens, const void* d_proofs, size_t n_plain, const void* d_plain_cards,
                               void* d_out_plain, void* d_out_index, void* d_token_status, void* d_card_status);

/* ---- dealing and seating in batches: masking / remasking with their proofs, and the tables' aggregate keys
 * [REF mod.rs:151-298; examples/round.rs:228-262]
 * Before the first shuffle every card of the open deck is masked with a Chaum-Pedersen proof and every player verifies all of them;
 * before that, every player's key comes with a Schnorr proof and a table's aggregate key is the sum of its players' keys.  One call
 * carries the cards, or the players, of many tables.  mask is remask of (O, card) [REF remasking.rs:10-22], so `kind` covers
 * mask / verify_mask / remask / verify_remask:
 *   MP_DEAL_MASK     inputs = C plaintext cards (one wire point each)     fs_init = Blake2s("Masking Proof")
 *   MP_DEAL_REMASK   inputs = C masked cards (c0 || c1)                   fs_init = Blake2s("Remasking Proof")
 *   keys       K wire points: the aggregate keys of the tables of the call      key_index  C uint32: key_index[c] < K names the key of card c
 * mp_mask_batch (whoever deals): out_masked[c] = in + (r G, r pk) with in = (O, card) for MP_DEAL_MASK, and out_proofs[c] the "sigma
 * transcript v2" proof for the bases (G, pk), the publics (r G, r pk) and the witness r = factors[c] -- the bytes of mp_msm / mp_remask_batch
 * followed by mp_sigma_prove_batch on that statement; one window table of pk for r pk and the commitment.  prover_seeds: C x 32 fresh
 * random bytes.  status[c]: 0, MP_ERR_BAD_ENCODING (key or input point not canonical, not on the curve or -- subject to
 * mp_set_subgroup_check -- outside the prime-order subgroup; factor >= q) or MP_ERR_BAD_ARGUMENT (key_index >= K); a lane whose status is
 * not 0 gives zero bytes.
 * mp_verify_mask_batch (every player): the publics (masked.c0 - in.c0, masked.c1 - in.c1) are computed on the device; status[c] = the word
 * of mp_sigma_verify_batch for that statement (0 or 6 "Chaum-Pedersen"), MP_ERR_BAD_ENCODING (key, input point, masked point or commitment
 * not canonical, not on the curve or -- subject to mp_set_subgroup_check -- outside the subgroup; response >= q) or MP_ERR_BAD_ARGUMENT
 * (key_index >= K, whatever else is wrong with the lane).
 * Limits: 1 <= C, K <= 1 048 576 (MP_ERR_BAD_ARGUMENT for the call otherwise).  Keyed and keyless tables alike (of the parameters only G
 * is used); never coalesced.
 * mp_verify_mask_batch_dev: the same with every pointer a DEVICE pointer -- d_inputs may be the d_out_decks of a prover -- enqueued on the
 * context's stream; d_status is final after mp_sync, and the buffers stay untouched until then.
 * mp_aggregate_keys_batch (seating): `tables` tables of P players each, lane l = table * P + seat; keys, proofs (1 point + 1 scalar) and
 * fs_init ([l][32] = Blake2s("Key Ownership Proof" || player_public_info), as mp_sigma_verify_batch takes it) per lane.  player_status[l] =
 * the word of mp_sigma_verify_batch(nbases = 1) on (G, keys[l]): 0, 5 "Schnorr Identification" or MP_ERR_BAD_ENCODING; table_status[k] =
 * the first player status of the table that is not 0, in seat order (the reference stops at the first bad proof); out_keys[k] = the sum of
 * the table's keys as a canonical wire point if table_status[k] == 0, zero bytes otherwise.  The keys are summed as given: that they are
 * distinct is the caller's to check, as in the reference.  Limits: 1 <= P, 1 <= tables, tables * P <= 1 048 576. */
#define MP_DEAL_MASK 0
#define MP_DEAL_REMASK 1
int mp_mask_batch(mp_table* t, int kind, size_t K, const uint8_t* keys, size_t C, const uint32_t* key_index, const uint8_t* inputs,
                  const uint8_t* factors, const uint8_t* prover_seeds, uint8_t* out_masked, uint8_t* out_proofs, int32_t* status);
int mp_verify_mask_batch(mp_table* t, int kind, size_t K, const uint8_t* keys, size_t C, const uint32_t* key_index, const uint8_t* inputs,
                         const uint8_t* masked, const uint8_t* proofs, int32_t* status);
int mp_verify_mask_batch_dev(mp_table* t, int kind, size_t K, const void* d_keys, size_t C, const void* d_key_index, const void* d_inputs,
                             const void* d_masked, const void* d_proofs, void* d_status);
int mp_aggregate_keys_batch(mp_table* t, size_t tables, uint32_t P, const uint8_t* keys, const uint8_t* proofs, const uint8_t* fs_init,
                            uint8_t* out_keys, int32_t* player_status, int32_t* table_status);
/* mp_aggregate_keys_ragged_batch: tables of different sizes in one call.  first: tables + 1 uint32 offsets (a host array, with the rules
 * of mp_unmask_ragged_batch's): table k seats the lanes first[k] .. first[k+1] - 1, at least one, first[tables] <= 1 048 576 lanes in all.
 * Everything else as mp_aggregate_keys_batch, per table; with first[k] = k * P the outputs are its bytes and words. */
int mp_aggregate_keys_ragged_batch(mp_table* t, size_t tables, const uint32_t* first, const uint8_t* keys, const uint8_t* proofs,
                                   const uint8_t* fs_init, uint8_t* out_keys, int32_t* player_status, int32_t* table_status);

/* ---- secrets drawn on the device from seeds: shuffle witnesses and player keys
 * [REF examples/round.rs:265-266, examples/parameter_selection.rs:38-39, mod.rs:123-130: Fr::rand(rng) / sample_vector(rng, N), then
 * Permutation::new(rng, N)]
 * Every secret the calls above consume -- masking factors, permutations, secret keys -- can be drawn where it is used, from one 32-byte
 * seed per proof (or per player), bit for bit what this stream gives on a CPU.  "mpshuffle secret stream v1", for seed[32], S scalars
 * and a permutation of length P:
 *     key  = BLAKE2s-256("mpshuffle secret stream v1" || seed)            (the 26 tag bytes, then the 32 seed bytes)
 *     rng  = ChaCha20Rng::from_seed(key)                                  (64-bit block counter from 0, stream 0: the prover's word stream)
 *     s_k  = Fr::rand(rng), k = 0 .. S-1                                  (arkworks 0.3: 4 u64, limb 0 first; the top 256 - bits(q) bits cleared;
 *                                                                          accepted iff < q; the accepted limbs ARE the Montgomery form, so the
 *                                                                          scalar is limbs * 2^-256 mod q)
 *     perm = [0 .. P-1]; for i = P-1 down to 1: j = rng.next_u64() % (i + 1); swap(perm[i], perm[j])
 * The scalars come first, then the permutation [REF parameter_selection.rs:38-39].  A candidate of Fr::rand is 8 stream words, so the
 * scalars sit on a grid of half blocks; the next_u64 draws follow directly behind the last candidate (accepted, by construction), low
 * word first -- they begin at word 0 or at word 8 of a 16-word block.  `%` is the full 64-bit remainder.  perm is a wire permutation:
 * out[i] = in[perm[i]].  The tag keeps the stream apart from the prover's own randomness, which is ChaCha20Rng::from_seed(seed) untagged:
 * ONE seed per proof feeds both.  A seed is 32 bytes of fresh CSPRNG output, used once: whoever knows it knows the witness, and two
 * shuffles from one seed are the same shuffle.  protocol.secret_stream (mental-poker_amd/protocol.py) is the CPU statement.
 * mp_sample_secrets_batch: L seeds -> out_scalars [L][S] wire scalars, out_perms [L][P] uint32; either may be NULL when its count is 0.
 * Limits: 1 <= L <= 1 048 576, S <= 4 096, P <= 4 096, not both 0 (MP_ERR_BAD_ARGUMENT for the call otherwise).  _dev: device pointers,
 * enqueued on the context's stream, final after mp_sync.  (Dealing: the factors of mp_mask_batch are a call with P = 0.)
 * mp_shuffle_and_remask_batch_seeded[_dev]: the witness of proof b is the stream of seeds[b] with S = P = N (masking factors, then the
 * permutation) and its prover seed is seeds[b] itself; bytes and status words are exactly those of mp_shuffle_and_remask_batch[_keys][_dev]
 * on that witness with prover_seeds = seeds.  shared_keys / d_keys: NULL = the table's key, otherwise one key per proof as in _batch_keys.
 * The witness is sampled into workspace of the context and goes nowhere else unless out_perms ([B][N] uint32) / out_factors ([B][N] wire
 * scalars) are given (either may be NULL).  The host form uploads decks and seeds (and keys) only; B <= 1 048 576 for the _dev form.
 * mp_keygen_batch [REF mod.rs:123-149]: sk_k = the single scalar of the stream of seeds[k] (S = 1, P = 0), pk_k = sk_k G from the table's
 * fixed-base table -- the bytes of mp_msm; with fs_init ([K][32], as mp_aggregate_keys_batch takes it; NULL = no proofs, out_proofs unused)
 * also the Schnorr proof of key ownership under the prover seed seeds[k] -- the bytes of mp_sigma_prove_batch(nbases = 1) on (G, pk, sk).  The
 * secret key does not pass through the host between sampler and prover.  1 <= K <= 1 048 576; status[k]: 0 or < 0.
 * All of them hold the context's lock; none is coalesced. */
int mp_sample_secrets_batch(mp_table* t, size_t L, const uint8_t* seeds, uint32_t S, uint32_t P, uint8_t* out_scalars, uint32_t* out_perms);
int mp_sample_secrets_batch_dev(mp_table* t, size_t L, const void* d_seeds, uint32_t S, uint32_t P, void* d_out_scalars, void* d_out_perms);
int mp_shuffle_and_remask_batch_seeded(mp_table* t, size_t B, const uint8_t* shared_keys, const uint8_t* decks, const uint8_t* seeds,
                                       uint8_t* out_decks, uint8_t* out_proofs, int32_t* status, uint32_t* out_perms, uint8_t* out_factors);
int mp_shuffle_and_remask_batch_seeded_dev(mp_table* t, size_t B, const void* d_keys, const void* d_decks, const void* d_seeds,
                                           void* d_out_decks, void* d_out_proofs, void* d_status, void* d_out_perms, void* d_out_factors);
int mp_keygen_batch(mp_table* t, size_t K, const uint8_t* seeds, const uint8_t* fs_init, uint8_t* out_keys, uint8_t* out_secret_keys,
                    uint8_t* out_proofs, int32_t* status);

/* ---- screening the sigma verifiers with grouped bucket equations (opt-in, off by default) -------------------------------------------
 * mp_unmask_batch[_dev], mp_verify_mask_batch[_dev], mp_aggregate_keys_batch and mp_sigma_verify_batch (and the ragged forms of the first
 * and the third, whose groups of consecutive lanes do not care where a card or a table ends) check every proof on a plan of its
 * own: per lane about 3 x (51 + 15) additions and 500 doublings.  With the screen on, the checks z g_i - c a_i - A_i = O of a GROUP of
 * consecutive lanes are added up -- each check with a weight of its own, two per Chaum-Pedersen lane, one per Schnorr lane -- into ONE
 * multi-scalar multiplication on the bucket pipeline of the shuffle verifier (a lane is five points of it where one base is the table's
 * G, about 18-33 additions each; G itself is one fixed-base term per group).  The weights are Fr::rand of ChaCha20(Blake2s(...)) over a
 * digest of every lane of the group -- bases, publics, commitments AND the response z, which the proof's own transcript never absorbs --,
 * so an error in one lane cannot cancel against another's except with probability ~2^-250; no host randomness is involved.  A group
 * whose equation fails, or that holds a lane already refused (encoding, subgroup, argument), is re-verified lane by lane on the per-proof
 * path -- its lanes only --, so every status word and every output byte is what the unscreened call gives; no honest lane is refused by
 * the screen alone.  Subgroup and curve tests stay per point, before the screen.
 *   lanes_per_group   0 = off (the default); MP_SIGMA_SCREEN_AUTO = sized by points like the groups of mp_set_group_verify (equations
 *                     for the split pipeline when the call brings enough points, honouring mp_set_bucket_bits / mp_set_bucket_split;
 *                     64 equations for the one-wave-per-window kernel below that; calls too small for groups of 16 lanes stay per
 *                     proof); any other value = lanes per group (the last group of a call may be short).  A value whose equation
 *                     cannot fit one bucket job (6 x lanes > 589 824 points) is MP_ERR_BAD_ARGUMENT.
 *   min_lanes         calls with fewer lanes keep the per-proof path.
 * On a curve with a cofactor (MP_CURVE_BLS12_377) the screen runs only while mp_set_subgroup_check is on: without the per-point test a
 * weighted sum and a per-proof check can disagree on points with a low-order component; with the test off every call takes the
 * per-proof path.
 * The _dev forms: with the screen on, a screened call WAITS ONCE for a 4-byte flag (as mp_verify_shuffle_batch_dev does under merged
 * verification), and once more for one word per group if some group failed; with the screen off they never wait.
 * mp_sigma_screen_stats: counters since the last mp_set_sigma_screen -- [0] lanes that went through a screening equation, [1] group
 * equations evaluated, [2] groups that failed, [3] lanes re-verified on the per-proof path.  Both calls hold the context's lock. */
#define MP_SIGMA_SCREEN_AUTO 0xFFFFFFFFu
int mp_set_sigma_screen(mp_table* t, uint32_t lanes_per_group, size_t min_lanes);
int mp_sigma_screen_stats(const mp_table* t, uint64_t out[4]);

/* ---- canonical serialisation (arkworks-0.3 `CanonicalSerialize` / `CanonicalDeserialize`, compressed) ----------------------
 * Every associated type of the trait is CanonicalSerialize + CanonicalDeserialize [REF src/lib.rs:45-71], and the reference's
 * harness measures `proof.serialized_size()` [REF examples/parameter_selection.rs:95]: these are the conversions between those
 * byte strings and the engine's wire v1.  Host work (no context, no GPU); deserialisation validates like ark-ec (canonical x, x on
 * the curve, prime-order subgroup on curves with a cofactor, scalars < q) and costs one square root per point.
 *   Fr 32 B LE | point: x LE in ceil((bits+2)/8) bytes, bit 7 of the last byte = (y > -y), bit 6 = infinity | Vec<T>: u64 LE length
 *   MaskedCard = 2 points; deck = Vec<MaskedCard>; Parameters { m, n, enc { G }, commit { Vec ck, H }, gen } [REF mod.rs:37-43];
 *   proof: elements in wire-v1 order, one Vec per vector-valued element (upstream's struct lives in the un-vendored dependency,
 *   so sizes are exact for this grouping; byte-compatibility with upstream's layout is not claimed).
 * Sizes: caller allocates; errors: MP_ERR_BAD_ENCODING (invalid data) / MP_ERR_BAD_ARGUMENT. */
size_t mp_serialized_point_size(int curve_id);                               /* 32 (STARK, bn254), 33 (secp256k1), 48 (BLS12-377) */
size_t mp_serialized_deck_size(int curve_id, size_t cards);
size_t mp_serialized_params_size(int curve_id, uint32_t n);
size_t mp_serialized_proof_size(int curve_id, uint32_t m, uint32_t n);      /* = ZKProofShuffle::serialized_size() */
int mp_points_serialize(int curve_id, size_t count, const uint8_t* wire_points, uint8_t* out);
int mp_points_deserialize(int curve_id, size_t count, const uint8_t* data, uint8_t* out_wire_points);
int mp_deck_serialize(int curve_id, size_t cards, const uint8_t* wire_deck, uint8_t* out);
int mp_deck_deserialize(int curve_id, const uint8_t* data, size_t len, size_t max_cards, uint8_t* out_wire_deck, size_t* out_cards);
int mp_params_serialize(int curve_id, uint32_t m, uint32_t n, const uint8_t* raw_params, uint8_t* out);
int mp_params_deserialize(int curve_id, const uint8_t* data, size_t len, size_t max_n, uint32_t* m, uint32_t* n, uint8_t* out_raw_params);
int mp_proof_serialize(int curve_id, uint32_t m, uint32_t n, const uint8_t* proof_wire, uint8_t* out);
int mp_proof_deserialize(int curve_id, uint32_t m, uint32_t n, const uint8_t* data, size_t len, uint8_t* out_proof_wire);
/* The same conversion ON THE DEVICE for the bulk data (round 4): decks that arrive as arkworks bytes go to HBM as they are -- half the
 * bytes of wire v1 over PCIe -- and are decompressed there, one lane per point, the square root as a windowed walk through the 2-Sylow
 * subgroup of the base field (4 512 squarings on the STARK prime, whose p - 1 has 2-adicity 192; the host path needs ~10^4), with the
 * validation of the host functions above: canonical x, flags, x on the curve, prime-order subgroup where there is a cofactor.  All
 * pointers are DEVICE pointers; the kernel is enqueued on the context's stream (mp_sync, or any later call on the context, orders
 * behind it).  d_status receives 0 or MP_ERR_BAD_ENCODING: one int32 per point (mp_points_deserialize_dev: `count` compressed points
 * back to back) / per deck (mp_deck_deserialize_dev: `decks` serialised Vec<MaskedCard> of `cards` cards each, back to back, every
 * one mp_serialized_deck_size bytes with its u64 length in front); a failing point leaves an all-zero wire point.  The output of
 * mp_deck_deserialize_dev is what mp_shuffle_and_remask_batch_dev / mp_verify_shuffle_batch_dev take as d_decks. */
int mp_points_deserialize_dev(mp_ctx* ctx, size_t count, const void* d_data, void* d_out_wire_points, void* d_status);
int mp_deck_deserialize_dev(mp_ctx* ctx, size_t decks, size_t cards, const void* d_data, void* d_out_wire_decks, void* d_status);
/* The other three conversions of a prove-or-verify round trip on the device, in batches.  Same rules: DEVICE pointers, the context's
 * lock, enqueued on the context's stream, final after mp_sync or any later call on the context; d_status is zeroed by the call and
 * receives 0 or MP_ERR_BAD_ENCODING, one int32 per unit; a null pointer or a zero count is MP_ERR_BAD_ARGUMENT and enqueues nothing.
 *   mp_points_serialize_dev   `count` wire points -> mp_serialized_point_size bytes each, the bytes of mp_points_serialize: all-zero wire
 *                             bytes are the point at infinity, the sign bit is 2y > p; only the range of x and y is checked (as on the
 *                             host), a coordinate >= p leaves an all-zero slot and -1 in the point's status word.
 *   mp_deck_serialize_dev     `decks` wire decks of `cards` cards (<= 4096) -> Vec<MaskedCard> of mp_serialized_deck_size bytes each, back
 *                             to back, u64 length in front: what mp_deck_deserialize_dev reads.  Status per deck.  The input may be the
 *                             prover's d_out_decks.
 *   mp_proof_serialize_dev    `B` wire proofs of mp_proof_size_curve bytes -> mp_serialized_proof_size bytes each, the bytes of
 *                             mp_proof_serialize.  Status per proof; scalars are copied as they are (the host does not judge them here).
 *   mp_proof_deserialize_dev  the inverse, with the validation of mp_proof_deserialize: every Vec length, every point as
 *                             mp_points_deserialize_dev validates one, every scalar < q.  A proof reads 0 iff mp_proof_deserialize accepts
 *                             its bytes, and then the wire bytes are the same.  Every element is converted on its own: in a proof that
 *                             reads -1 the refused points and scalars are zero bytes and the valid elements are converted (the host form
 *                             stops at the first error).  The output is what mp_verify_shuffle_batch_dev takes as d_proofs. */
int mp_points_serialize_dev(mp_ctx* ctx, size_t count, const void* d_wire_points, void* d_out, void* d_status);
int mp_deck_serialize_dev(mp_ctx* ctx, size_t decks, size_t cards, const void* d_wire_decks, void* d_out, void* d_status);
int mp_proof_serialize_dev(mp_ctx* ctx, uint32_t m, uint32_t n, size_t B, const void* d_proofs_wire, void* d_out, void* d_status);
int mp_proof_deserialize_dev(mp_ctx* ctx, uint32_t m, uint32_t n, size_t B, const void* d_data, void* d_out_proofs_wire, void* d_status);
/* HOST buffers, conversion on the device: one upload, mp_deck_deserialize_dev / mp_proof_deserialize_dev, one download; bytes and
 * statuses are theirs, and the call returns with both in place.  For a caller without device buffers: bulk data never meets the host's
 * square root.  Buffers from mp_host_alloc are copied asynchronously, pageable ones work too.  These calls are never coalesced; their
 * device staging stays with the context. */
int mp_decks_deserialize_batch(mp_ctx* ctx, size_t decks, size_t cards, const uint8_t* data, uint8_t* out_wire_decks, int32_t* status);
int mp_proofs_deserialize_batch(mp_ctx* ctx, uint32_t m, uint32_t n, size_t B, const uint8_t* data, uint8_t* out_proofs_wire, int32_t* status);

/* ---- measurement hooks ---------------------------------------------------------------------------------------
 * With profiling on, every kernel launch is bracketed by HIP events on the context's stream;
 * mp_profile_report writes "name count total_ms items\n" lines (and resets) -- bench.py's roofline source; items = threads launched (waves
 * for the wave-cooperative kernels, (equation, window) items for k_bucket_msm), summed over the launches of that name. */
int mp_profile_enable(mp_ctx* ctx, int on);
int mp_profile_report(mp_ctx* ctx, char* buf, size_t buf_len);
/* static work census of one prove / verify for this table: number of scalar*point terms and point operations */
int mp_work_census(mp_table* t, uint64_t* prove_terms, uint64_t* verify_terms, uint64_t* prove_point_ops,
                   uint64_t* verify_point_ops);

/* static plan statistics for this table (what one proof costs, per kernel class); out[16]:
 *  [0..5]  prove : fixed terms, var terms, fixed jobs, var jobs, table bases, combine terms
 *  [6..11] verify: same six
 *  [12] variable-base windows per scalar  [13] fixed-base windows per scalar  [14] N  [15] reserved */
int mp_plan_stats(mp_table* t, uint64_t out[16]);

#ifdef __cplusplus
}
#endif
#endif /* MPSHUFFLE_H */
