/*
 * bbs_sign_amd -- C ABI of the MI355X-native batched BBS+ engine.
 *
 * This is the drop-in boundary for the hot path of hashcloak/bbs_sign: the `core_*` level of the
 * reference (the narrowest seam that isolates all heavy arithmetic and that the reference's own
 * tests call directly, src/tests/core_sign_tests.rs:53-64).  Each entry point names the reference
 * function it replaces.  Plain pointers and sizes only; no exceptions cross this boundary.
 *
 * Data formats (both curves):
 *   Fp / Fr element : canonical value < modulus, LITTLE-endian bytes (48 B for BLS12-381 Fp,
 *                     32 B otherwise) == ark-ff `into_bigint().to_bytes_le()`.
 *   G1 affine       : x || y (2 * fp_bytes); the identity is encoded as all-zero bytes.
 *   G2 affine       : x.c0 || x.c1 || y.c0 || y.c1 (4 * fp_bytes) + a separate identity flag.
 *   scalar          : 32 B LE, must be < r (else per-item status BBS_ST_NONCANONICAL).
 *   ragged arrays   : a flat buffer + an offsets array of n+1 uint64 (item i owns
 *                     [off[i], off[i+1]) in units of elements: scalars, indexes or bytes).
 *
 * Per-item status (int8): mirrors the reference's Result<bool|T, Error>:
 *     1  Ok(true) / Ok(value)        0  Ok(false)
 *   < 0  the Err variant, a reference panic, or an input the reference's types cannot hold.
 * -128 and -127 are internal "not decided yet" states: the library never returns them -- a fetch that finds one
 * fails with BBS_E_STATE instead (an item no kernel decided must not read as Ok(true)).
 * Function return: 0 on success, BBS_E_* on a batch-level failure (nothing was computed).
 */
#ifndef BBS_SIGN_AMD_H
#define BBS_SIGN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BBS_CURVE_BLS12_381 0
#define BBS_CURVE_BN254 1

#define BBS_FR_BYTES 32

/* per-item status codes */
#define BBS_ST_TRUE 1
#define BBS_ST_FALSE 0
/* SignatureError (src/sign.rs:24-28) / ProofGenError (src/proof_gen.rs:59-75) */
#define BBS_ST_INVALID_MESSAGE_AND_GENERATORS_LENGTH (-1)
#define BBS_ST_INVALID_DISCLOSED_INDICES_LENGTH (-2)
#define BBS_ST_INVALID_DISCLOSED_INDEX (-3)
#define BBS_ST_INVALID_RANDOM_SCALARS_AND_UNDISCLOSED_INDICES_LENGTH (-4)
#define BBS_ST_INVALID_UNDISCLOSED_INDICES_LENGTH (-5)
#define BBS_ST_INVALID_INDICES_AND_MESSAGES_LENGTH (-6)
/* KeyGenError (src/key_gen.rs:34-42) */
#define BBS_ST_INVALID_KEY_MATERIAL_LENGTH (-7)
#define BBS_ST_INVALID_KEY_INFO_LENGTH (-8)
#define BBS_ST_INVALID_SECRET_KEY (-9)
/* reference panics */
#define BBS_ST_PANIC_SK_PLUS_E_ZERO (-20)     /* src/sign.rs:129 unwrap on inverse of 0 */
#define BBS_ST_PANIC_R2_ZERO (-21)            /* src/proof_gen.rs:346 unwrap on inverse of 0 */
#define BBS_ST_PANIC_INDEX_OUT_OF_BOUNDS (-22)/* src/proof_verify.rs:177-179 commitments[i] */
#define BBS_ST_PANIC_DST_TOO_LONG (-23)       /* src/utils/utilities_helper.rs:46-52 */
#define BBS_ST_PANIC_ELL_TOO_BIG (-24)        /* src/utils/utilities_helper.rs:46-48: expand_message of more than 255 * 32 bytes
                                                (seeded random scalars only: more than 170 scalars for one item) */
/* inputs arkworks' types cannot represent */
#define BBS_ST_NONCANONICAL (-40)             /* scalar >= r or coordinate >= p */
#define BBS_ST_NOT_ON_CURVE (-41)            /* also: not in the prime-order subgroup (codec) */
#define BBS_ST_INVALID_ENCODING (-42)        /* octet string of the wrong shape / forbidden identity or zero */
#define BBS_ST_NO_RESOURCES (-43)            /* bbs_issuer_* only: the context of this item's message count could not be set
                                              * up (device memory, or every resident context busy at the context limit); the
                                              * item was NOT computed -- the other items of the call were; retry later */
#define BBS_ST_UNKNOWN_KEY (-44)             /* keyed entry points only: the item's key index is >= the key set's size or names a
                                              * key that bbs_ctx_set_public_keys refused; decided at ingest, never computed */
#define BBS_ST_NO_SECRET_KEY (-45)           /* keyed sign only: the item's key index names an accepted key of the key set that was
                                              * registered public-only (no secret half); decided at ingest, never computed */

/* batch-level errors */
#define BBS_OK 0
#define BBS_E_ARG (-100)
#define BBS_E_HIP (-101)
#define BBS_E_STATE (-102)       /* generators / public key / secret key not set; or an item left undecided */
#define BBS_E_PUBLIC_KEY (-103)  /* public key not on the twist or not of order r */
#define BBS_E_NO_DEVICE (-104)
#define BBS_E_NOMEM (-105)
#define BBS_E_UNSUPPORTED (-106) /* reserved: operation not available for this curve */
#define BBS_E_NO_RESOURCES (-107)/* the hardware-queue budget of the device is spent (bbs_runtime_queue_budget): nothing was created */

typedef struct bbs_ctx bbs_ctx;
typedef struct bbs_job bbs_job;

/* ------------------------------------------------------------------------------------------
 * Context: one per (curve, GPU, issuer key, generator set).  Holds the device-resident
 * fixed-base window tables of {P1, Q1, H_1..H_L}, the domain-hash midstate and the Miller-loop
 * line tables of the issuer key.  Thread-compatible (one call at a time per context).
 * ------------------------------------------------------------------------------------------ */
size_t bbs_fp_bytes(int curve);
const char* bbs_version(void);
/* Hash of the sources (every file under bbs_sign_amd/csrc and this header) the library was built from; bbs_sign_amd/build.py rebuilds
 * when it differs from the tree's (a prebuilt library travels with the tree: staleness is judged by content). */
const char* bbs_source_hash(void);
/* GPU_MAX_HW_QUEUES as the process environment has it (0 = unset).  The library sets 20 when it is loaded unless the
 * variable is already set; the HIP runtime reads it at its own initialisation, so the setting only takes effect if
 * this library was loaded before the process's first HIP call ("Build / deployment"). */
int bbs_runtime_hw_queues(void);
/* For a process that cannot arrange that (its first HIP call -- any torch import that touches the GPU -- comes before this
 * library is loaded: the runtime's pool is then 4 hardware queues, several jobs share one, 1.30 M proof_verify/s instead
 * of 1.50 M): up to k job streams per device get a hardware queue OF THEIR OWN (streams created with an all-ones
 * compute-unit mask, which the runtime does not draw from the pool) -- 1.50 M/s whatever GPU_MAX_HW_QUEUES says
 * (profiles/r04_f_dedicated_queues.log; on the present library profiles/auto_queues_ab.log).
 * THE DEFAULT IS AUTOMATIC: if this function is never called and BBS_DEDICATED_QUEUES is not in the environment, the
 * library makes up what the runtime's pool lacks of its own 20, at most 12 -- a pool of 4 gives 12, 14 gives 6, 20 or
 * more none.  The pool it goes by is the EFFECTIVE one, from what it found when it was loaded: a GPU_MAX_HW_QUEUES somebody
 * else had set counts as set; its own 20 counts only if the runtime had not started yet, otherwise -- and when that cannot
 * be told -- the runtime's default of 4 (bbs_runtime_queue_report shows what was assumed and granted).
 * k = 0: OFF, never overridden; k >= 1: at most k (12 is a good value, 16 the most accepted).  k, asked for or automatic, is a
 * WISH: every hardware queue reserves scratch memory for the largest kernel frame it has run, pooled + dedicated queues x
 * that frame is a budget, and past it the runtime first collapses and then ABORTS the process -- so per device the library
 * keeps   dedicated streams + min(GPU_MAX_HW_QUEUES as the environment has it, pooled streams) <= bbs_runtime_queue_budget's
 * total,   counted in streams it has really created, grants a dedicated stream only where room is left for the effective pool
 * beside it, and serves further streams from the pool.  A wrong guess of the pool costs speed, never the abort.
 * Call before the first context is created (streams are recycled); BBS_DEDICATED_QUEUES=k in the environment does the same
 * (1 means 12).  Caveat: such streams synchronise with the legacy default stream (the runtime offers no non-blocking flag
 * for them): a process that also runs its own kernels on stream 0 BESIDE the jobs -- torch and RCCL work on the default
 * stream -- serialises them with the jobs.  Such a host sets 0 and loads this library before its first HIP call instead. */
int bbs_runtime_set_dedicated_queues(int k);
/* The hardware-queue budget of a device, as the library enforces it: *scratch_bytes_per_lane = the largest kernel frame of
 * this library (every kernel is asked at start-up), *total = hardware queues (pooled + dedicated) that frame allows within
 * 8.5 % of the device's memory (queues x bytes per lane x 64 lanes x wave slots; 25 on MI355X at 1.8 KB), *pool =
 * GPU_MAX_HW_QUEUES as the environment has it (4 when unset), *dedicated_cap = max(0, total - pool).  If the POOL alone exceeds
 * the budget (an explicit GPU_MAX_HW_QUEUES=32) the library creates at most `total` streams: a job that gets none of its own
 * shares its context's stream and runs its side-stream stages in order on it, and bbs_ctx_create fails with
 * BBS_E_NO_RESOURCES once even the context's stream cannot be had -- slower or refused, never the runtime's abort.  Any
 * pointer may be NULL.  BBS_E_NO_DEVICE for a device that does not exist. */
int bbs_runtime_queue_budget(int device_id, int* total, int* pool, int* dedicated_cap, size_t* scratch_bytes_per_lane);
/* What the library decided and granted on a device so far: *mode = the dedicated-queue setting (-1 automatic, 0 off, k >= 1
 * asked for), *effective_pool = the pool the runtime is taken to use (see bbs_runtime_set_dedicated_queues), *dedicated_made /
 * *pooled_made = streams with a hardware queue of their own / from the runtime's pool that the library has created on the
 * device and not destroyed (in use or waiting to be reused).  Any pointer may be NULL.  BBS_E_NO_DEVICE for a device that does
 * not exist. */
int bbs_runtime_queue_report(int device_id, int* mode, int* effective_pool, int* dedicated_made, int* pooled_made);
int bbs_device_count(void);
size_t bbs_device_free_bytes(int device_id);          /* device memory free right now (0: no such device) */

int bbs_ctx_create(int curve, int device_id, bbs_ctx** out);
void bbs_ctx_destroy(bbs_ctx* ctx);
/* device memory of the context's tables (fixed-base window tables, line tables, constants, the per-length domain
 * prefixes of bbs_ctx_set_mixed_lengths / bbs_ctx_set_mixed_lengths_gen and the per-(key, length) prefixes of bbs_ctx_set_keyed_mixed_lengths), in bytes */
size_t bbs_ctx_table_bytes(const bbs_ctx* ctx);

/* window width (bits) of the fixed-base tables, 4..22, or 0 (THE DEFAULT) = chosen at bbs_ctx_set_generators from the
 * memory free on the device: the widest of 20 / 16 / 12 / 8 whose tables fit 1/32 of it and 8 GiB (32 messages on an empty
 * MI355X: 16 bits, 2 GB; ask for 20 explicitly where one issuer may have 26 GB for +3.5 %) -- and, if that
 * allocation fails all the same (the free figure is a snapshot: other ranks or processes on the device, fragmentation),
 * the next narrower width, down to 8, before BBS_E_NOMEM; takes effect at the next bbs_ctx_set_generators, which changes
 * nothing of the context unless it succeeds.  Digits are SIGNED: table bytes = (count+1) * ceil(256/w) * 2^(w-1) * 2 * limb bytes of
 * an Fp element (56 on BLS12-381, 40 on BN254) -- for 32 messages 26 GB at w = 20 (1.45 M proof_verify/s, 8.0 M sign/s),
 * 2 GB at 16 (1.30 M, 7.3 M), 172 MB at 12 (1.30 M, 6.1 M), 16 MB at 8 (1.18 M, 4.4 M). */
int bbs_ctx_set_window_bits(bbs_ctx* ctx, int bits);

/* Subgroup vouching (off by default).  The reference's point types (ark-ec `Affine`, built by `deserialize_compressed`
 * or `Affine::new`, src/proof_gen.rs:29, src/sign.rs:18) can only hold members of the prime-order subgroup; this ABI
 * takes raw coordinates and by default computes exactly what the reference's double-and-add would for ANY on-curve
 * point -- with ONE exception, core_proof_gen: Abar e and Abar e~ (src/proof_gen.rs:255-258) are computed as the multiples
 * (r1 r2 e mod r) A and (r1 r2 e~ mod r) A of the signature's own point, which is the reference's value for every A in the
 * prime-order subgroup (all that the reference's types can hold) and for the identity; for an on-curve A OUTSIDE the
 * subgroup -- a signature that cannot verify -- the proof's Bbar, T1 and what follows from them differ from the
 * reference's (tests: check_proof_gen_unusual_points pins what is computed instead).  vouched = 1 promises that every G1 point later handed to core_verify / core_proof_verify / core_proof_gen (and the generators given to
 * bbs_ctx_set_generators) through this context is in the subgroup (true for everything that came out of bbs_*_from_octets*, which check it): on BLS12-381
 * the variable-base multiplications of those paths then use the GLV endomorphism split (half the doublings).  Results
 * are identical for such inputs; for on-curve points outside the subgroup they are unspecified.  BN254 has cofactor 1
 * (every on-curve point is in the subgroup), so there the split is always on and this setting changes nothing.
 * Takes effect for jobs uploaded afterwards. */
int bbs_ctx_set_points_in_subgroup(bbs_ctx* ctx, int vouched);

/* Latency form of a job.  A batch can be laid out for the least WORK (the throughput form: T1 = Bbar*c + Abar*e^ + D*r1^,
 * src/proof_verify.rs:163-164, as ONE joint windowed chain on one lane per item; both Miller loops of an item's pairing
 * product on one six-lane group with shared squarings) or for the shortest CRITICAL PATH (the latency form: the three
 * multiplications on three lanes, summed afterwards; the two Miller loops on separate wavefronts, multiplied before the
 * final exponentiation).  Same group elements and booleans; the latency form is ~25 % shorter for a batch that has the
 * chip to itself and costs ~15 % more instructions, so it loses once several batches are in flight.
 *   enabled = 0: never; 1: always; 2: AUTO (the default) -- a job gets the latency form iff at most one other job is alive
 *   ON THE DEVICE when it is created (upload / submit; jobs of every context of the process count: the contexts of one
 *   bbs_issuer, or a BLS12-381 and a BN254 context side by side, share the chip), i.e. a serving loop that keeps many
 *   batches in flight runs in the throughput form, a caller that verifies one batch at a time gets the short path
 *   without asking.
 * Takes effect for jobs created afterwards. */
int bbs_ctx_set_latency_mode(bbs_ctx* ctx, int enabled);
/* Fixed-base sums (the generators' multiples: B of sign / verify / proof_gen, the fixed part of T2 of proof_verify) as
 * ONE tree of affine additions per item with one shared inversion per level, instead of eight chains of mixed Jacobian
 * additions: fewer field multiplications, the same group element, bit-identical results.  Needs work memory of about
 * 90 bytes x table points (messages + 2) x windows per item of a job.  EXPERIMENTAL and off by default: in its present
 * form it is not faster (measured); today it covers proof_verify and bbs_g1_msm_batch.  Applies to jobs
 * created afterwards. */
int bbs_ctx_set_fixed_base_tree(bbs_ctx* ctx, int enabled);
/* Mixed message counts on ONE context (off by default; with it off nothing changes anywhere).  The reference picks its
 * generators by the item's own length on every call (create_generators of messages.len + 1, src/verify.rs:30-35; of
 * commitments + disclosed indexes + 1, src/proof_verify.rs:40-43), and generator i does not depend on the count: the
 * tables of a context with L message generators contain those of every shorter length.  enabled = 1: every SINGLE-KEY verify
 * and proof_verify entry point of the context -- core, octets and wire forms; _upload, _submit and _batch -- accepts item i
 * with its own count l_i, 0 <= l_i <= L (verify: its messages; proof_verify: its commitments + disclosed indexes).  The
 * status of item i is exactly what a context made with generators[0 .. l_i] (same key, api_id and modes) gives that item
 * alone: the checks and their order are unchanged, only "l != L" becomes "l > L" (still -1); -3, -6, -22, -23, -40, -41 and
 * -42 are decided against the item's own l_i.  Composes with both job forms, batch verification, subgroup vouching, the
 * fixed-base tree and every window width.  Costs L + 1 domain prefixes (about 370 bytes each) of device memory, counted in
 * bbs_ctx_table_bytes, rebuilt by bbs_ctx_set_generators and the key setters.  Applies to jobs created afterwards; a job keeps
 * what it was created with.
 * NOT covered: the keyed entry points look at bbs_ctx_set_keyed_mixed_lengths (below), not at this switch; with this switch on
 * and that one off they return BBS_E_STATE and enqueue nothing; sign and proof_gen do not look at this switch (theirs is bbs_ctx_set_mixed_lengths_gen, below) and keep deciding
 * l != L as -1 whatever this one says; bbs_issuer and bbs_pool keep one context per count; the C++ wrapper and the Rust shim do not expose the switch. */
int bbs_ctx_set_mixed_lengths(bbs_ctx* ctx, int enabled);
/* Mixed message counts for the PRODUCING side (off by default; with it off nothing changes anywhere).  The reference picks its
 * generators by the item's own count in sign and proof_gen too (src/sign.rs:44-49, src/proof_gen.rs:91-96).  enabled = 1: every
 * sign and proof_gen entry point of the context -- bbs_core_sign_*, bbs_sign_octets_*, bbs_sign_wire_*, bbs_core_proof_gen_*,
 * bbs_proof_gen_octets_*, bbs_proof_gen_wire_*; _upload, _batch and _submit; both job forms -- takes item i with its own message
 * count l_i, 0 <= l_i <= L.  The status AND the output bytes of item i are, bit for bit, what a context made with
 * generators[0 .. l_i] (same key, api_id, modes and random scalars) gives that item alone: the checks and their order are
 * unchanged, only "l != L" becomes "l > L" (still -1); -2, -3, -4, -20, -21, -23 and -40 are decided against the item's own
 * l_i -- a disclosed index with l_i <= index < L is -3.  proof_gen delivers exactly l_i - r_i commitments (an octet string of
 * exactly the fixed-length proof's size); the contract on the number of random scalars, 5 + l_i - r_i (BBS_E_ARG for the call),
 * was per item already.
 * Independent of bbs_ctx_set_mixed_lengths and bbs_ctx_set_keyed_mixed_lengths: verify and proof_verify never look at this
 * switch.  It shares the L + 1 domain prefixes with bbs_ctx_set_mixed_lengths: they are built while either switch is on, counted
 * ONCE in bbs_ctx_table_bytes, and rebuilt by bbs_ctx_set_generators, bbs_ctx_set_secret_key and bbs_ctx_set_public_key, so
 * every order of set-up ends in the same outputs.  Applies to jobs created afterwards; a job keeps the stages it was created
 * with.  BBS_E_ARG for a NULL ctx.
 * NOT covered: the keyed proof_gen and keyed sign entry points look at bbs_ctx_set_keyed_mixed_lengths (below), not at this
 * switch; with this switch on and that one off they return BBS_E_STATE and enqueue nothing; bbs_issuer and bbs_pool keep one
 * context per count; the C++ wrapper and the Rust shim do not expose the switch. */
int bbs_ctx_set_mixed_lengths_gen(bbs_ctx* ctx, int enabled);
/* Seeded random scalars for proof_gen, drawn on the device (off by default; with it off nothing changes anywhere).  enabled = 1:
 * every proof_gen entry point of the context -- the nine single-key and the four keyed exports: core, octets and wire forms;
 * _upload, _batch and _submit; both job forms; bbs_ctx_set_mixed_lengths_gen and bbs_ctx_set_keyed_mixed_lengths on or off --
 * reads its random_scalars / rnd_off pair as SEEDS, in one of two shapes:
 *   per-item seeds (rnd_off != NULL): item i's seed is the BYTES random_scalars[rnd_off[i] .. rnd_off[i + 1]); offsets in
 *       bytes, any length, 0 included;
 *   job seed (rnd_off == NULL): random_scalars is ONE job seed of which exactly 32 bytes are read (fewer readable bytes cannot
 *       be checked); item i's seed is job_seed || I2OSP(i, 8), i the item's position in the call.
 * Item i's scalars are seeded_random_scalars(seed_i, dst, 5 + l_i - r_i) of the reference (src/utils/core_utilities.rs:84-100:
 * expand_message_xmd(SHA-256) of 48 bytes per scalar, each through FromOkm), r_i counted before deduplication as the reference
 * sizes its draw and l_i the item's own count in a mixed-length job, and dst[0 .. dst_len) is copied into the context.  The
 * status AND the output bytes of an item are, bit for bit, those of the call with the switch off that is given those scalars,
 * but for two codes the reference's draw (proof_gen.rs:145-149) raises before proof_init's checks (:229-239).  After -2 and -3
 * and before every other code of core_proof_gen an item is BBS_ST_PANIC_ELL_TOO_BIG when 5 + l_i - r_i > 170 (ell > 255) and
 * BBS_ST_PANIC_DST_TOO_LONG when dst_len > 255 (utilities_helper.rs:46-52, in that order).  What is decided ahead of core_proof_gen stays ahead: the codes
 * of signature decoding (wire form), msg_to_scalars' -23, and BBS_ST_UNKNOWN_KEY, which overrides everything in a keyed job.  An
 * item that is decided before the draw draws nothing and its seed is not read.  The contract of the switch-off call on the
 * number of random scalars (BBS_E_ARG) does not apply; the staged image carries the seeds instead of the scalars.
 * Memory: the stored dst, counted in bbs_ctx_table_bytes.  Applies to jobs created afterwards; a job keeps what it was created
 * with.  BBS_E_ARG for a NULL ctx, or a NULL dst with dst_len > 0.
 * SECURITY: a seed is a secret exactly as the scalars are, and it must never serve two different proofs: the same job seed in
 * two jobs repeats nonces, which gives away e and the hidden messages.  The caller owns freshness.
 * NOT covered: bbs_issuer_*, bbs_pool_*, the C++ wrapper and the Rust shim do not expose the switch. */
int bbs_ctx_set_seeded_random_scalars(bbs_ctx* ctx, int enabled, const uint8_t* dst, size_t dst_len);
/* Mixed message counts for the KEYED entry points (off by default; with it off nothing changes anywhere, the BBS_E_STATE above
 * included).  enabled = 1: every keyed verify and proof_verify job created from now on -- the eight bbs_*_keyed_* exports: core
 * and wire forms, _submit and _batch, both job forms -- takes item i under its own key key_index[i] AND with its own count l_i,
 * 0 <= l_i <= L.  The status of item i is, bit for bit, what a single-key context made with generators[0 .. l_i], that key and
 * the same api_id and modes gives that item alone: the checks and their order are those of bbs_ctx_set_mixed_lengths ("l != L"
 * becomes "l > L", still -1; -3, -6, -22, -23, -40, -41, -42 against the item's own l_i), and behind them an unknown or refused
 * key index is BBS_ST_UNKNOWN_KEY whatever those checks decided, as in every keyed job.  Keyed jobs keep ignoring batch
 * verification.
 * Memory: one domain prefix per (key, length), (L + 1) * 368 bytes per key of the set, refused keys included (12 144 bytes at
 * L = 32, beside the key's 29 KB line table), counted in bbs_ctx_table_bytes while the switch is on.  The prefixes are built on
 * host threads when the switch is turned on (for the keys of the set) and by every registration call while it is on (for the
 * keys it appends; the old rows are copied on the device), so any order of bbs_ctx_set_generators, registration and this call
 * ends in the same verdicts; bbs_ctx_set_generators clears the key set and with it the prefixes, and while the switch is on a
 * context without a key set is one with an empty set: every item is BBS_ST_UNKNOWN_KEY (with the switch off: BBS_E_STATE, as
 * before).  Turning the switch off releases them.  BBS_E_NOMEM / BBS_E_HIP leave the switch as it was.
 * Independent of bbs_ctx_set_mixed_lengths: single-key jobs never look at this switch, keyed jobs look at that one only to
 * return BBS_E_STATE when it is on and this one is off.  Applies to jobs created afterwards; a job keeps the stages, the key set
 * and the prefixes it was created with, whatever is switched, appended or replaced later.  BBS_E_ARG for a NULL ctx.
 * Keyed proof_gen (bbs_*proof_gen*_keyed_*, below) takes mixed counts by this switch too: the same prefixes, and the output
 * bytes of item i are those of bbs_ctx_set_mixed_lengths_gen on that single-key context.  So does keyed sign
 * (bbs_*sign*_keyed_*, below).
 * NOT covered: bbs_issuer and bbs_pool do not route through it; the C++ wrapper and the Rust shim do not expose the switch. */
int bbs_ctx_set_keyed_mixed_lengths(bbs_ctx* ctx, int enabled);

/* Form of the Miller-loop line tables (on by default).  Both G2 arguments of a pairing product are fixed per key, so the
 * lines of a table can be scaled by the inverse of their constant term c (an element of Fp2: the final exponentiation
 * removes it) and a line costs the pairing kernel two sparse products instead of three.  enabled = 1: every table of the
 * context -- BP2's, the public key's, the key set's -- is kept in that unit form; a key whose walk meets c = 0 (a line
 * through the twist's origin) has none, and while the context holds such a key all its tables are kept in the (c, nl) form,
 * so such a key keeps working.  enabled = 0: the (c, nl) form throughout.  Verdicts are the same in both forms; the switch
 * exists to measure one against the other in one build and to test the fallback.  The call rebuilds the tables on the host
 * (BBS_E_NOMEM / BBS_E_HIP as registration) and, like a change of key, is meant for a context without jobs in flight: a
 * keyed job that was created before the switch fails its pairing stage instead of mixing forms.  BBS_E_ARG for a NULL ctx. */
int bbs_ctx_set_unit_lines(bbs_ctx* ctx, int enabled);

/* Batch verification for core_proof_verify and core_verify (off by default).  When enabled, the n two-pairing
 * products of a batch (src/proof_verify.rs:112-115, src/verify.rs:88-92) are replaced by 16 products over random
 * linear combinations of the items' G1 arguments (sum rho_i * Abar_i, sum rho_i * Bbar_i; for verify
 * sum rho_i * A_i, sum rho_i * (e_i A_i - B_i)) with 16 independent 8-bit coefficients rho_i per item derived
 * from a secret seed (bucket-method multi-scalar multiplication on the device), taken over the items that passed
 * every earlier check (a proof_verify job in its latency form combines beside the challenge check instead of behind it:
 * over the structurally valid items); only if one of those combined checks fails are the items still pending checked
 * one by one.  The booleans
 * equal the reference's except with probability 2^-128 per batch.  seed32 = NULL draws the seed from the operating
 * system; a caller-supplied seed must be secret and fresh.  Takes effect for jobs uploaded afterwards. */
int bbs_ctx_set_batch_verification(bbs_ctx* ctx, int enabled, const uint8_t* seed32);

/* Batch verification for the KEYED entry points, per issuer key (off by default; with it off nothing changes anywhere).
 * Independent of bbs_ctx_set_batch_verification: single-key jobs never look at this switch and keyed jobs keep ignoring that
 * one.  enabled = 1: in every keyed verify and proof_verify job created afterwards -- the eight bbs_*verify*_keyed_* exports:
 * core and wire forms, _submit and _batch, both job forms -- a key that at least min_items_per_key of the job's items name
 * forms a GROUP.  For the group of key k the library checks  e(sum rho_i Abar_i, W_k) e(sum rho_i Bbar_i, -BP2) == 1  (verify:
 * A_i and e_i A_i - B_i) over the group's items that passed every earlier check, as 16 independent 8-bit combinations
 * (rho_i from the secret seed and the item's index, as above), each one ordinary item of the keyed pairing kernel under key k.
 * If all 16 pass, every such item of the group is true except with probability 2^-128; otherwise the group's items are
 * decided one by one by the exact kernel, as are the items of keys below the threshold.  The statuses are therefore those of
 * the switch-off job, and a failing key costs only its own group.
 * min_items_per_key = 0: the library's default (256, the smallest group size at which the combination was measured to win:
 * DESIGN.md 8); any value >= 1 is taken as given (groups below the default are slower combined than alone on the measured
 * loop, and a group of 16 or fewer items costs more pairing products combined than alone: small values are for tests).
 * seed32 as for bbs_ctx_set_batch_verification; the context has ONE seed: enabling either switch sets it.  A job draws its
 * coefficients once, when it is created (as a job of bbs_ctx_set_batch_verification does): bbs_job_run again repeats the same
 * combination, so the 2^-128 bound is per job, not per run -- an input that is to be checked afresh is uploaded afresh.
 * Composes with bbs_ctx_set_keyed_mixed_lengths, subgroup vouching and both line-table forms.  Costs no stream and no hardware
 * queue: everything runs on the job's main stream.  BBS_E_ARG for a NULL ctx.
 * NOT covered: one combined check across keys; a narrower-window form for small groups; bbs_issuer and bbs_pool do not route
 * through it; the C++ wrapper and the Rust shim do not expose the switch or the report. */
int bbs_ctx_set_keyed_batch_verification(bbs_ctx* ctx, int enabled, const uint8_t* seed32, size_t min_items_per_key);

/* generators = [Q1, H_1 .. H_L] (count = L+1 affine G1 points) and the api_id they belong to:
 * the `generators: &[E::G1]` and `api_id: &[u8]` arguments of every reference core_* function
 * (src/sign.rs:63-69, src/verify.rs:53-60, src/proof_gen.rs:116-125, src/proof_verify.rs:64-73). */
int bbs_ctx_set_generators(bbs_ctx* ctx, const uint8_t* generators_affine, size_t count,
                           const uint8_t* api_id, size_t api_id_len);

/* issuer public key (`pk: PublicKey<E>`, src/key_gen.rs:12-15). */
int bbs_ctx_set_public_key(bbs_ctx* ctx, const uint8_t* pk_affine, int is_identity);
/* issuer secret key (`&self` of core_sign, src/sign.rs:63); also sets pk = sk * BP2
 * (src/key_gen.rs:83-90, src/sign.rs:81). */
int bbs_ctx_set_secret_key(bbs_ctx* ctx, const uint8_t* sk32);
int bbs_ctx_get_public_key(bbs_ctx* ctx, uint8_t* pk_affine_out, int* is_identity_out);
/* ark-serialize compressed public key as hashed into the domain (96 B BLS / 64 B BN254). */
int bbs_ctx_get_public_key_compressed(bbs_ctx* ctx, uint8_t* out, size_t cap, size_t* len_out);

/* ------------------------------------------------------------------------------------------
 * Batched core operations.  `*_upload` stages the batch in page-locked memory, copies it to HBM with one
 * asynchronous copy and enqueues the ingest kernel -- the reference's checks in the reference's order, range
 * checks and unpacking run on the device -- and returns a device-resident job; `bbs_job_run` enqueues the
 * kernels on the job's streams (asynchronous); `bbs_job_wait` blocks; `bbs_job_fetch_*` copies results back.
 * The one-shot `*_batch` functions do all of it; `*_submit` is the asynchronous one-shot form.
 * Order of the per-item codes in every record form (core_proof_verify, core_verify, core_sign, core_proof_gen): the
 * reference's own errors and panics first, in the reference's order (proof_verify: -3, -6, -1, -23, -22; verify and sign:
 * -1, -23; proof_gen: -2, -3, -1, -4, -23); then BBS_ST_NONCANONICAL for ANY coordinate >= p or scalar >= r of the item,
 * wherever it stands (record, commitments, messages, disclosed messages, random scalars); then BBS_ST_NOT_ON_CURVE.
 * ------------------------------------------------------------------------------------------ */

/* core_proof_verify (src/proof_verify.rs:64-116 with proof_verify_init :119-188).
 * proofs_fixed: n records of  a_bar || b_bar || d (3 G1 affine) || e_cap || r1_cap || r3_cap ||
 * challenge (4 scalars)  == 6*fp_bytes + 128 bytes each (src/proof_gen.rs:29-39).
 * commitments / disclosed_msgs: scalars, ragged; disclosed_idx: uint64 indexes, ragged, caller
 * order is significant exactly as in the reference (src/proof_verify.rs:18). */
int bbs_core_proof_verify_upload(bbs_ctx* ctx, size_t n, const uint8_t* proofs_fixed,
                                 const uint8_t* commitments, const uint64_t* commit_off,
                                 const uint8_t* disclosed_msgs, const uint64_t* dmsg_off,
                                 const uint64_t* disclosed_idx, const uint64_t* didx_off,
                                 const uint8_t* headers, const uint64_t* hdr_off,
                                 const uint8_t* ph, const uint64_t* ph_off, bbs_job** job_out);
int bbs_core_proof_verify_batch(bbs_ctx* ctx, size_t n, const uint8_t* proofs_fixed,
                                const uint8_t* commitments, const uint64_t* commit_off,
                                const uint8_t* disclosed_msgs, const uint64_t* dmsg_off,
                                const uint64_t* disclosed_idx, const uint64_t* didx_off,
                                const uint8_t* headers, const uint64_t* hdr_off,
                                const uint8_t* ph, const uint64_t* ph_off, int8_t* status);

/* Asynchronous form of bbs_core_proof_verify_batch, for a stream of batches from ONE submitting thread per GPU: the
 * inputs are staged in page-locked memory (the caller's input buffers may be reused as soon as the call returns), then
 * ONE host-to-device copy, the validation / unpacking kernel (the reference's checks of src/proof_verify.rs:139-150 and
 * the range checks run on the device), the verification kernels and the copy of the statuses back are enqueued; the
 * call returns without waiting for the device, so several submitted batches are in flight together.
 * bbs_job_wait(job) blocks until `status` (n entries; must stay valid until then) has been written -- it returns
 * BBS_E_STATE, and writes nothing, if any item was left undecided (fail closed); then bbs_job_free(job). */
int bbs_core_proof_verify_submit(bbs_ctx* ctx, size_t n, const uint8_t* proofs_fixed,
                                 const uint8_t* commitments, const uint64_t* commit_off,
                                 const uint8_t* disclosed_msgs, const uint64_t* dmsg_off,
                                 const uint64_t* disclosed_idx, const uint64_t* didx_off,
                                 const uint8_t* headers, const uint64_t* hdr_off,
                                 const uint8_t* ph, const uint64_t* ph_off, int8_t* status, bbs_job** job_out);

/* core_proof_verify from the WIRE: the n proofs as octet strings (compress(Abar) || compress(Bbar) || compress(D) || e^ ||
 * r1^ || r3^ || m^_1 .. m^_U || c, scalars 32 bytes big-endian: the form of src/tests/test_vector.rs:199-260; ragged,
 * oct_off: n + 1 byte offsets) instead of decoded records.  Decompression (square roots), on-curve and prime-order-subgroup
 * checks and the scalar range checks run on the device in front of the same pipeline; the per-item status is what
 * bbs_proof_from_octets followed by bbs_core_proof_verify_batch would give: BBS_ST_INVALID_ENCODING (shape, identity
 * point), BBS_ST_NONCANONICAL, BBS_ST_NOT_ON_CURVE (also: outside the subgroup) before the reference's own checks.  The
 * disclosed messages are scalars, as for bbs_core_proof_verify_batch.  Because every point has been subgroup-checked, the
 * variable-base terms use the GLV split (BLS12-381) without bbs_ctx_set_points_in_subgroup.
 * Order: the codes of bbs_proof_from_octets in its order (below: the shape, the first failing point, the proof's scalars);
 * then the reference's -3, -6, -1, -23, -22; then BBS_ST_NONCANONICAL for a disclosed message >= r. */
int bbs_proof_verify_octets_submit(bbs_ctx* ctx, size_t n, const uint8_t* proof_octets, const uint64_t* oct_off,
                                   const uint8_t* disclosed_msgs, const uint64_t* dmsg_off,
                                   const uint64_t* disclosed_idx, const uint64_t* didx_off,
                                   const uint8_t* headers, const uint64_t* hdr_off,
                                   const uint8_t* ph, const uint64_t* ph_off, int8_t* status, bbs_job** job_out);
int bbs_proof_verify_octets_batch(bbs_ctx* ctx, size_t n, const uint8_t* proof_octets, const uint64_t* oct_off,
                                  const uint8_t* disclosed_msgs, const uint64_t* dmsg_off,
                                  const uint64_t* disclosed_idx, const uint64_t* didx_off,
                                  const uint8_t* headers, const uint64_t* hdr_off,
                                  const uint8_t* ph, const uint64_t* ph_off, int8_t* status);
/* The reference's PUBLIC proof_verify (src/proof_verify.rs:19-61) for contexts of a fixed number of messages, in one
 * call: proof octet strings and the disclosed messages as RAW BYTES.  Message t of the batch is
 * msg_bytes[msg_byte_off[t] .. msg_byte_off[t + 1]) (t counts the disclosed messages of all items in order);
 * msg_item_off[i] .. msg_item_off[i + 1] are the messages of item i (n + 1 entries, in messages; as with every offset
 * array of this header they need not start at zero: a window into larger arrays is passed by pointing into them).  msg_to_scalars
 * (interface_utilities.rs:76-88, dst = api_id || "MAP_MSG_TO_SCALAR_AS_HASH_") runs on the device in front of the checks;
 * statuses as bbs_proof_verify_octets_* on the hashed messages (BBS_ST_PANIC_DST_TOO_LONG for an item with disclosed
 * messages when that dst exceeds 255 bytes, as the reference's expand_message panics). */
int bbs_proof_verify_wire_submit(bbs_ctx* ctx, size_t n, const uint8_t* proof_octets, const uint64_t* oct_off,
                                 const uint8_t* msg_bytes, const uint64_t* msg_byte_off, const uint64_t* msg_item_off,
                                 const uint64_t* disclosed_idx, const uint64_t* didx_off,
                                 const uint8_t* headers, const uint64_t* hdr_off,
                                 const uint8_t* ph, const uint64_t* ph_off, int8_t* status, bbs_job** job_out);
int bbs_proof_verify_wire_batch(bbs_ctx* ctx, size_t n, const uint8_t* proof_octets, const uint64_t* oct_off,
                                const uint8_t* msg_bytes, const uint64_t* msg_byte_off, const uint64_t* msg_item_off,
                                const uint64_t* disclosed_idx, const uint64_t* didx_off,
                                const uint8_t* headers, const uint64_t* hdr_off,
                                const uint8_t* ph, const uint64_t* ph_off, int8_t* status);

/* core_verify (src/verify.rs:53-93).  signatures: n records  A (G1 affine) || e (scalar). */
int bbs_core_verify_upload(bbs_ctx* ctx, size_t n, const uint8_t* signatures,
                           const uint8_t* messages, const uint64_t* msg_off,
                           const uint8_t* headers, const uint64_t* hdr_off, bbs_job** job_out);
int bbs_core_verify_batch(bbs_ctx* ctx, size_t n, const uint8_t* signatures,
                          const uint8_t* messages, const uint64_t* msg_off,
                          const uint8_t* headers, const uint64_t* hdr_off, int8_t* status);
/* asynchronous form, as bbs_core_proof_verify_submit: bbs_job_wait(job) delivers `status`, then bbs_job_free(job) */
int bbs_core_verify_submit(bbs_ctx* ctx, size_t n, const uint8_t* signatures,
                           const uint8_t* messages, const uint64_t* msg_off,
                           const uint8_t* headers, const uint64_t* hdr_off, int8_t* status, bbs_job** job_out);

/* verify from the wire: n signature octet strings of fp_bytes + 32 octets each, compress(A) || I2OSP(e, 32) (the byte
 * string of src/tests/test_vector.rs:188-191), decompressed, subgroup- and range-checked on the device in front of
 * core_verify.  status[i] = what bbs_signature_from_octets gives when it fails (malformed / not on the curve or in the
 * subgroup / identity / e = 0 or >= r, in the order given at bbs_signature_from_octets), else what core_verify gives.
 * _submit as bbs_core_verify_submit. */
int bbs_verify_octets_submit(bbs_ctx* ctx, size_t n, const uint8_t* signature_octets,
                             const uint8_t* messages, const uint64_t* msg_off,
                             const uint8_t* headers, const uint64_t* hdr_off, int8_t* status, bbs_job** job_out);
int bbs_verify_octets_batch(bbs_ctx* ctx, size_t n, const uint8_t* signature_octets,
                            const uint8_t* messages, const uint64_t* msg_off,
                            const uint8_t* headers, const uint64_t* hdr_off, int8_t* status);

/* The reference's PUBLIC verify (src/verify.rs:18-50) for a context's number of messages in one call: signature octet
 * strings and the messages as RAW BYTES (layout of the message arrays as bbs_proof_verify_wire_submit); msg_to_scalars on
 * the device.  Statuses as bbs_verify_octets_* on the hashed messages. */
int bbs_verify_wire_submit(bbs_ctx* ctx, size_t n, const uint8_t* signature_octets,
                           const uint8_t* msg_bytes, const uint64_t* msg_byte_off, const uint64_t* msg_item_off,
                           const uint8_t* headers, const uint64_t* hdr_off, int8_t* status, bbs_job** job_out);
int bbs_verify_wire_batch(bbs_ctx* ctx, size_t n, const uint8_t* signature_octets,
                          const uint8_t* msg_bytes, const uint64_t* msg_byte_off, const uint64_t* msg_item_off,
                          const uint8_t* headers, const uint64_t* hdr_off, int8_t* status);

/* ------------------------------------------------------------------------------------------
 * Keyed verification: ONE context verifies items of MANY issuers.  The reference takes the public key per call
 * (src/verify.rs:18-50, src/proof_verify.rs:19-61); here a context holds a KEY SET beside its generators and every item of a
 * keyed batch names its key by index.  The fixed-base tables, which depend only on the generators and api_id, are shared by
 * all keys; a key costs its W line table and its domain midstate (~30 KB of device memory on BLS12-381).
 * A key set GROWS BY APPENDING (bbs_ctx_add_public_keys*): keys already in the set keep their index and their bytes, so a
 * verifier that meets its issuers one after another prepares every key once.  A key is prepared -- decoded, checked to be on
 * the twist and of order r, its line table and midstate built -- on up to 16 host threads, then uploaded.  (A device stage
 * that prepares a key per lane exists and gives the same entries byte for byte -- bbs_selftest_key_entries -- but no call
 * uses it until it has been timed against the host threads.)  What is allocated: one device array of exactly (keys in the
 * set) entries of bbs_selftest_key_entry_bytes(curve) bytes, nothing spare; an append allocates the new array, copies the old
 * entries device to device and frees the old array with its last holder.
 * ------------------------------------------------------------------------------------------ */
/* n_keys issuer public keys (affine records as bbs_ctx_set_public_key; is_identity may be NULL = none).  key_status[k] (may
 * be NULL): 1, or BBS_ST_NOT_ON_CURVE for a key bbs_ctx_set_public_key would refuse (not on the twist / not of order r; a
 * record with a coordinate >= p counts as not on the twist: a record has no code of its own for it).
 * Replaces the context's previous key set (a new empty set, then an append); n_keys = 0 clears it.  Independent of
 * bbs_ctx_set_public_key.  Needs the generators (BBS_E_STATE); bbs_ctx_set_generators clears the key set.  A set is immutable
 * once built and every keyed job holds the set it was created with: replacing it or appending to it while jobs are in flight
 * does not change their results.  BBS_E_NOMEM if the set does not fit on the device (the previous set stays). */
int bbs_ctx_set_public_keys(bbs_ctx* ctx, size_t n_keys, const uint8_t* pk_affine, const int8_t* is_identity,
                            int8_t* key_status);
/* Append n keys to the context's key set (to an empty set when there is none); their indexes are [*first_index, *first_index
 * + n).  Entries already in the set keep their index and their bytes.  Jobs in flight keep the set they were created with.
 * Refused keys still occupy an index (key_status as bbs_ctx_set_public_keys; items naming them get BBS_ST_UNKNOWN_KEY).  n = 0
 * only reports the set's size in *first_index.  BBS_E_ARG for a NULL first_index, or a NULL pk_affine or key_status with n >
 * 0; BBS_E_STATE without generators; on any failure the set stays as it was. */
int bbs_ctx_add_public_keys(bbs_ctx* ctx, size_t n, const uint8_t* pk_affine, const int8_t* is_identity,
                            int8_t* key_status, uint32_t* first_index);
/* The same for keys as they travel: n compressed octet strings of 2 * fp_bytes each, the format bbs_public_key_to_octets
 * writes.  key_status[k]: 1, BBS_ST_NONCANONICAL or BBS_ST_NOT_ON_CURVE -- what bbs_public_key_from_octets returns for that
 * string (with 1 for BBS_OK); the identity encoding is an accepted identity key.  pk_affine_out (n records, may be NULL) and
 * is_identity_out (n flags, may be NULL) receive the decoded keys, zero for a refused key. */
int bbs_ctx_add_public_keys_octets(bbs_ctx* ctx, size_t n, const uint8_t* pk_octets, int8_t* key_status,
                                   uint8_t* pk_affine_out, int8_t* is_identity_out, uint32_t* first_index);
/* keys in the context's key set, refused ones included (0: no set) */
size_t bbs_ctx_public_key_count(const bbs_ctx* ctx);
/* Keyed forms of bbs_core_proof_verify_*, bbs_proof_verify_wire_*, bbs_core_verify_* and bbs_verify_wire_*: the arguments
 * of the un-keyed form plus key_index (n entries) after n.  For an item whose key_index names an accepted key the status is
 * what the un-keyed form gives on a context with the same generators, api_id, window bits and modes and that key set by
 * bbs_ctx_set_public_key; for an index >= the set's size or naming a refused key it is BBS_ST_UNKNOWN_KEY.  BBS_E_STATE
 * without generators; without a key set (unless bbs_ctx_set_keyed_mixed_lengths is on: then a missing set is the empty set
 * and every item is BBS_ST_UNKNOWN_KEY); and on a context with bbs_ctx_set_mixed_lengths on unless
 * bbs_ctx_set_keyed_mixed_lengths is on too (then every item has its own count, see there).  BBS_E_ARG for a NULL key_index
 * with n > 0.  Batch verification (bbs_ctx_set_batch_verification) does not apply: every item gets its own pairing product.
 * The _submit forms return ordinary jobs (bbs_job_wait, bbs_jobs_wait_any, bbs_job_free). */
int bbs_core_proof_verify_keyed_submit(bbs_ctx* ctx, size_t n, const uint32_t* key_index, const uint8_t* proofs_fixed,
                                       const uint8_t* commitments, const uint64_t* commit_off,
                                       const uint8_t* disclosed_msgs, const uint64_t* dmsg_off,
                                       const uint64_t* disclosed_idx, const uint64_t* didx_off,
                                       const uint8_t* headers, const uint64_t* hdr_off,
                                       const uint8_t* ph, const uint64_t* ph_off, int8_t* status, bbs_job** job_out);
int bbs_core_proof_verify_keyed_batch(bbs_ctx* ctx, size_t n, const uint32_t* key_index, const uint8_t* proofs_fixed,
                                      const uint8_t* commitments, const uint64_t* commit_off,
                                      const uint8_t* disclosed_msgs, const uint64_t* dmsg_off,
                                      const uint64_t* disclosed_idx, const uint64_t* didx_off,
                                      const uint8_t* headers, const uint64_t* hdr_off,
                                      const uint8_t* ph, const uint64_t* ph_off, int8_t* status);
int bbs_proof_verify_wire_keyed_submit(bbs_ctx* ctx, size_t n, const uint32_t* key_index, const uint8_t* proof_octets,
                                       const uint64_t* oct_off, const uint8_t* msg_bytes, const uint64_t* msg_byte_off,
                                       const uint64_t* msg_item_off, const uint64_t* disclosed_idx, const uint64_t* didx_off,
                                       const uint8_t* headers, const uint64_t* hdr_off,
                                       const uint8_t* ph, const uint64_t* ph_off, int8_t* status, bbs_job** job_out);
int bbs_proof_verify_wire_keyed_batch(bbs_ctx* ctx, size_t n, const uint32_t* key_index, const uint8_t* proof_octets,
                                      const uint64_t* oct_off, const uint8_t* msg_bytes, const uint64_t* msg_byte_off,
                                      const uint64_t* msg_item_off, const uint64_t* disclosed_idx, const uint64_t* didx_off,
                                      const uint8_t* headers, const uint64_t* hdr_off,
                                      const uint8_t* ph, const uint64_t* ph_off, int8_t* status);
int bbs_core_verify_keyed_submit(bbs_ctx* ctx, size_t n, const uint32_t* key_index, const uint8_t* signatures,
                                 const uint8_t* messages, const uint64_t* msg_off,
                                 const uint8_t* headers, const uint64_t* hdr_off, int8_t* status, bbs_job** job_out);
int bbs_core_verify_keyed_batch(bbs_ctx* ctx, size_t n, const uint32_t* key_index, const uint8_t* signatures,
                                const uint8_t* messages, const uint64_t* msg_off,
                                const uint8_t* headers, const uint64_t* hdr_off, int8_t* status);
int bbs_verify_wire_keyed_submit(bbs_ctx* ctx, size_t n, const uint32_t* key_index, const uint8_t* signature_octets,
                                 const uint8_t* msg_bytes, const uint64_t* msg_byte_off, const uint64_t* msg_item_off,
                                 const uint8_t* headers, const uint64_t* hdr_off, int8_t* status, bbs_job** job_out);
int bbs_verify_wire_keyed_batch(bbs_ctx* ctx, size_t n, const uint32_t* key_index, const uint8_t* signature_octets,
                                const uint8_t* msg_bytes, const uint64_t* msg_byte_off, const uint64_t* msg_item_off,
                                const uint8_t* headers, const uint64_t* hdr_off, int8_t* status);
/* ------------------------------------------------------------------------------------------
 * Verification under keys that ARRIVE WITH THE JOB: per-job key sets.  The keyed exports above serve a closed set of issuers
 * whose keys were registered beforehand.  These eight serve a verifier that learns the issuer key next to the proof: the call
 * passes the DISTINCT keys of the job as compressed octets (n_keys strings of 2 * fp_bytes bytes, the format
 * bbs_ctx_add_public_keys_octets takes) and key_index[i] names a key OF THIS CALL.  The job prepares its keys on the device as its
 * own first work -- one lane per key decodes the string, tests the twist and [r]Q, walks the Miller-loop line table and hashes
 * the domain midstate (and, with bbs_ctx_set_keyed_mixed_lengths on, one lane per (key, length) hashes the prefixes) -- on its
 * main stream in front of its ingest kernel, asynchronously like everything else of a job, into arrays it owns (counted by
 * bbs_job_device_bytes: per key the entry, 22 848 bytes of workspace on BLS12-381, a status byte, and (L + 1) prefixes of
 * 368 bytes in jobs of mixed counts) and releases with the job.  The context's key set is neither read nor changed; a context
 * without a public key or a key set serves these calls.  The key bytes are copied into the job's staging image by the call: the
 * caller's array is free when _submit returns.  The library does NOT deduplicate with the cache off: a key given twice is
 * prepared twice and is two keys.  The keys are prepared with the upload, as the ingest kernel runs with the upload: bbs_job_run on the same job
 * runs the stages again over the same prepared keys.
 * Arguments: those of the keyed twin with n_keys and pk_octets in front of key_index.
 * STATUS RULE: the status array is, bit for bit, what the keyed twin returns on a context with the same generators, api_id and
 * switches whose key set was built by bbs_ctx_add_public_keys_octets(pk_octets), given the same key_index and items.  So an
 * index >= n_keys is BBS_ST_UNKNOWN_KEY, a key registration would refuse (BBS_ST_NONCANONICAL, BBS_ST_NOT_ON_CURVE) makes its
 * items BBS_ST_UNKNOWN_KEY, the identity encoding is an accepted key, and everything else is decided as under that key alone.
 * Which keys were accepted is decided on the device: the host plans the job (pairing order, groups of keyed batch verification)
 * with every index < n_keys, and a gate behind the key stage decides the items of a refused key; they keep their slots and are
 * left out by status as every decided item is.
 * FAIL-CLOSED CASE: a key whose line walk meets a line through the twist's origin (c = 0) has no unit form.  Registration moves
 * the whole context to the (c, nl) form for such a key; a job cannot.  On a context in the unit form (the default) the items of
 * such a key get BBS_ST_UNKNOWN_KEY although bbs_job_key_statuses says 1 for it.  No key of order r is known to reach this;
 * register such a key (bbs_ctx_add_public_keys*) to use it.
 * BBS_E_ARG: NULL pk_octets with n_keys > 0, NULL key_index with n > 0, n_keys > 0xFFFFFFF0, a NULL status.  BBS_E_STATE: no
 * generators; bbs_ctx_set_mixed_lengths on without bbs_ctx_set_keyed_mixed_lengths (as the keyed twins).
 * Composition: both job forms, bbs_ctx_set_points_in_subgroup, both line forms, bbs_ctx_set_keyed_mixed_lengths (per-item
 * counts), bbs_ctx_set_keyed_batch_verification (groups form by the job's own key indexes; bbs_job_bv_report counts the groups of
 * accepted keys, bbs_job_bv_verdicts returns 16 flags for every group the host planned, refused keys included).
 * bbs_ctx_set_batch_verification is not looked at.
 * bbs_job_key_statuses: after bbs_job_wait, the per-key codes (1, BBS_ST_NONCANONICAL, BBS_ST_NOT_ON_CURVE) in the order of
 * pk_octets, copied from the device on request (nothing is added to a run); *n_out = n_keys; BBS_E_ARG where cap < n_keys;
 * BBS_E_STATE for a job without a key set of its own.
 * NOT covered: bbs_issuer, bbs_pool, the C++ wrapper and the Rust shim; keyed sign with job-local keys (proof_gen has them:
 * bbs_*proof_gen*_with_keys_* below); preparing a handful of keys on the host instead (one call of the key stage costs one walk
 * however few keys it brings); running the key stage beside the MSM stages on a side stream; a faster subgroup test by the
 * curve endomorphism; registration through the device stage. */
int bbs_core_proof_verify_with_keys_submit(bbs_ctx* ctx, size_t n, size_t n_keys, const uint8_t* pk_octets,
                                           const uint32_t* key_index, const uint8_t* proofs_fixed,
                                           const uint8_t* commitments, const uint64_t* commit_off,
                                           const uint8_t* disclosed_msgs, const uint64_t* dmsg_off,
                                           const uint64_t* disclosed_idx, const uint64_t* didx_off,
                                           const uint8_t* headers, const uint64_t* hdr_off,
                                           const uint8_t* ph, const uint64_t* ph_off, int8_t* status, bbs_job** job_out);
int bbs_core_proof_verify_with_keys_batch(bbs_ctx* ctx, size_t n, size_t n_keys, const uint8_t* pk_octets,
                                          const uint32_t* key_index, const uint8_t* proofs_fixed,
                                          const uint8_t* commitments, const uint64_t* commit_off,
                                          const uint8_t* disclosed_msgs, const uint64_t* dmsg_off,
                                          const uint64_t* disclosed_idx, const uint64_t* didx_off,
                                          const uint8_t* headers, const uint64_t* hdr_off,
                                          const uint8_t* ph, const uint64_t* ph_off, int8_t* status);
int bbs_proof_verify_wire_with_keys_submit(bbs_ctx* ctx, size_t n, size_t n_keys, const uint8_t* pk_octets,
                                           const uint32_t* key_index, const uint8_t* proof_octets,
                                           const uint64_t* oct_off, const uint8_t* msg_bytes, const uint64_t* msg_byte_off,
                                           const uint64_t* msg_item_off, const uint64_t* disclosed_idx, const uint64_t* didx_off,
                                           const uint8_t* headers, const uint64_t* hdr_off,
                                           const uint8_t* ph, const uint64_t* ph_off, int8_t* status, bbs_job** job_out);
int bbs_proof_verify_wire_with_keys_batch(bbs_ctx* ctx, size_t n, size_t n_keys, const uint8_t* pk_octets,
                                          const uint32_t* key_index, const uint8_t* proof_octets,
                                          const uint64_t* oct_off, const uint8_t* msg_bytes, const uint64_t* msg_byte_off,
                                          const uint64_t* msg_item_off, const uint64_t* disclosed_idx, const uint64_t* didx_off,
                                          const uint8_t* headers, const uint64_t* hdr_off,
                                          const uint8_t* ph, const uint64_t* ph_off, int8_t* status);
int bbs_core_verify_with_keys_submit(bbs_ctx* ctx, size_t n, size_t n_keys, const uint8_t* pk_octets,
                                     const uint32_t* key_index, const uint8_t* signatures,
                                     const uint8_t* messages, const uint64_t* msg_off,
                                     const uint8_t* headers, const uint64_t* hdr_off, int8_t* status, bbs_job** job_out);
int bbs_core_verify_with_keys_batch(bbs_ctx* ctx, size_t n, size_t n_keys, const uint8_t* pk_octets,
                                    const uint32_t* key_index, const uint8_t* signatures,
                                    const uint8_t* messages, const uint64_t* msg_off,
                                    const uint8_t* headers, const uint64_t* hdr_off, int8_t* status);
int bbs_verify_wire_with_keys_submit(bbs_ctx* ctx, size_t n, size_t n_keys, const uint8_t* pk_octets,
                                     const uint32_t* key_index, const uint8_t* signature_octets,
                                     const uint8_t* msg_bytes, const uint64_t* msg_byte_off, const uint64_t* msg_item_off,
                                     const uint8_t* headers, const uint64_t* hdr_off, int8_t* status, bbs_job** job_out);
int bbs_verify_wire_with_keys_batch(bbs_ctx* ctx, size_t n, size_t n_keys, const uint8_t* pk_octets,
                                    const uint32_t* key_index, const uint8_t* signature_octets,
                                    const uint8_t* msg_bytes, const uint64_t* msg_byte_off, const uint64_t* msg_item_off,
                                    const uint8_t* headers, const uint64_t* hdr_off, int8_t* status);
int bbs_job_key_statuses(bbs_job* job, int8_t* out, size_t cap, size_t* n_out);
/* ------------------------------------------------------------------------------------------
 * THE JOB-LOCAL KEY CACHE: prepared keys kept across the jobs of the eight exports above.  A verifier that resolves the issuer
 * per presentation sees the same issuers again and again; without the cache every job pays one walk of the key stage for keys
 * a job before it prepared and released.  bbs_ctx_set_job_key_cache with capacity_keys > 0 gives the context that many key
 * SLOTS on the device; the jobs of the eight exports uploaded afterwards look every key string up, prepare only the strings no
 * slot holds (the MISSES, by the same two kernels, into arrays of the job), copy them into their slots with one more small
 * kernel and read ALL their keys -- entries, statuses, prefixes per (key, length) -- from the cache's arrays.  0 (the default)
 * switches the cache off and drops it; with it off every job takes the uncached path, bit for bit.  A new capacity starts an empty
 * cache.
 * STATUS RULE: unchanged.  The statuses, bbs_job_key_statuses, bbs_job_bv_report and bbs_job_bv_verdicts of a cached job are, bit
 * for bit, those of the same call with the cache off: the host plans in the job's own key numbering (groups and verdict order
 * are the keyed twin's) and translates key -> slot where the job's words hold a key id.
 * LOOKUP: by the WHOLE compressed string of 2 * fp_bytes bytes, compared in full, never by a digest alone.  A refused string is
 * cached as refused under its own bytes, the identity encoding as the accepted key it is.  hits + misses == n_keys for every
 * cached job; a string given twice in one call is one miss (or one hit) the first time, a hit after that, and both indexes name
 * the same slot.
 * ORDER ACROSS JOBS: a string is entered when the job is planned, its slot carries an event recorded behind the copying kernel.
 * A later job on another stream that hits the slot before the event has completed waits for it ON THE DEVICE, in front of its
 * key gate; nothing waits on the host.  An upload that fails after claiming slots gives them back.
 * PINS AND EVICTION: every slot a job names is pinned from its upload until bbs_job_free (a job may be run again).  Slots for
 * misses come from the free slots first, then from the unpinned slots, least recently used first (a hit, and a pin by the job
 * being planned, count as use).  A job is BYPASSED -- takes the uncached path, correct and slower -- if n_keys > capacity, if its
 * misses outnumber the free and evictable slots, or if one of its strings is claimed by an upload another host thread has not
 * finished yet.
 * GENERATIONS: the cached entries depend on the generators and api_id, on the line form and on whether prefixes per
 * (key, length) are kept.  A job whose form differs from the cache's -- after bbs_ctx_set_generators, bbs_ctx_set_unit_lines, a
 * registration that moved the context to the (c, nl) form, bbs_ctx_set_keyed_mixed_lengths -- starts a new, empty generation; the
 * old one lives on through the jobs that hold it.
 * MEMORY: allocated by the first cached job, capacity * (entry + 1 + (L + 1) * 368 bytes under keyed mixed lengths; 0 otherwise):
 * about 41 KB per key on BLS12-381 at L = 32 with mixed counts.  BBS_E_NOMEM from that upload if it cannot be had.
 * The fail-closed case above is unchanged: a cached key without a unit form is refused by the gate of every job.
 * Key strings are public; what the cache reveals (through timing and the reports) is which issuers a context has seen.
 * bbs_ctx_set_job_key_cache: BBS_E_ARG for a NULL ctx or capacity_keys > 0xFFFFFFF0.
 * bbs_ctx_job_key_cache_report: capacity, slots that hold a string, slots pinned by jobs; hits, misses, evictions and bypassed
 * jobs counted since the context was created; device bytes of the current generation.  Any out-pointer may be NULL.
 * bbs_job_key_cache_report: hits and misses of this job (both 0 where the cache was off or the job was bypassed), *bypassed;
 * any out-pointer may be NULL; BBS_E_STATE for a job that did not come through one of the eight exports.
 * The four bbs_*proof_gen*_with_keys_* exports below go through the same generation of the cache (their own paragraph says how).
 * NOT covered: bbs_issuer, bbs_pool, the C++ wrapper and the Rust shim; keyed sign with job-local keys; a lookup on the device. */
int bbs_ctx_set_job_key_cache(bbs_ctx* ctx, size_t capacity_keys);
int bbs_ctx_job_key_cache_report(bbs_ctx* ctx, size_t* capacity, size_t* resident, size_t* pinned,
                                 uint64_t* hits, uint64_t* misses, uint64_t* evictions,
                                 uint64_t* bypassed_jobs, size_t* device_bytes);
int bbs_job_key_cache_report(bbs_job* job, uint32_t* hits, uint32_t* misses, int* bypassed);
/* Keyed forms of bbs_core_proof_gen_* and bbs_proof_gen_wire_*: ONE context derives proofs from signatures of MANY issuers.
 * The reference takes the public key per call (src/proof_gen.rs:78-113) and uses it in calculate_domain alone -- no pairing,
 * no W -- so a keyed item reads its key's domain midstate from the key set the keyed verify entry points use, and everything
 * else is the single-key job.  The arguments are those of the un-keyed form plus key_index (n entries) after n.  For an item
 * whose key_index names an accepted key (the identity key is one) the status AND the output bytes are, bit for bit, what the
 * un-keyed form gives that item alone on a context with the same generators, api_id, window bits, modes and random scalars and
 * that key set by bbs_ctx_set_public_key; for an index >= the set's size or naming a refused key the status is
 * BBS_ST_UNKNOWN_KEY whatever the other checks decided, and the item has no output (zero record, no octet string).  The
 * context's single public key is not needed and not looked at.  With bbs_ctx_set_keyed_mixed_lengths on, item i also has its
 * own count l_i <= L and its bytes are those of a single-key context made with generators[0 .. l_i].
 * BBS_E_STATE without generators; without a key set (unless bbs_ctx_set_keyed_mixed_lengths is on: then a missing set is the
 * empty set and every item is BBS_ST_UNKNOWN_KEY); and on a context with bbs_ctx_set_mixed_lengths_gen on unless
 * bbs_ctx_set_keyed_mixed_lengths is on too.  BBS_E_ARG for a NULL key_index with n > 0, a NULL status, and -- whatever the
 * item's key -- for an item whose number of random scalars is not 5 + l_i - r_i.  Both job forms; the _submit forms return
 * ordinary jobs.  A key costs its full entry (~30 KB on BLS12-381, the W line table included) although proof_gen reads only the
 * midstate: there is no cheaper registration for proof-only keys -- a holder-side service that meets its issuer keys next to
 * the credentials uses the bbs_*proof_gen*_with_keys_* exports below, which register nothing.
 * NOT covered: the octets (non-wire) keyed form and an _upload form; bbs_issuer, bbs_pool, the C++ wrapper and the Rust shim
 * do not route through these. */
int bbs_core_proof_gen_keyed_submit(bbs_ctx* ctx, size_t n, const uint32_t* key_index, const uint8_t* signatures,
                                    const uint8_t* messages, const uint64_t* msg_off,
                                    const uint64_t* disclosed_idx, const uint64_t* didx_off,
                                    const uint8_t* random_scalars, const uint64_t* rnd_off,
                                    const uint8_t* headers, const uint64_t* hdr_off,
                                    const uint8_t* ph, const uint64_t* ph_off,
                                    uint8_t* proofs_fixed_out, uint8_t* commitments_out,
                                    uint64_t* commit_off_out, int8_t* status, bbs_job** job_out);
int bbs_core_proof_gen_keyed_batch(bbs_ctx* ctx, size_t n, const uint32_t* key_index, const uint8_t* signatures,
                                   const uint8_t* messages, const uint64_t* msg_off,
                                   const uint64_t* disclosed_idx, const uint64_t* didx_off,
                                   const uint8_t* random_scalars, const uint64_t* rnd_off,
                                   const uint8_t* headers, const uint64_t* hdr_off,
                                   const uint8_t* ph, const uint64_t* ph_off,
                                   uint8_t* proofs_fixed_out, uint8_t* commitments_out,
                                   uint64_t* commit_off_out, int8_t* status);
int bbs_proof_gen_wire_keyed_submit(bbs_ctx* ctx, size_t n, const uint32_t* key_index, const uint8_t* signature_octets,
                                    const uint8_t* msg_bytes, const uint64_t* msg_byte_off, const uint64_t* msg_item_off,
                                    const uint64_t* disclosed_idx, const uint64_t* didx_off,
                                    const uint8_t* random_scalars, const uint64_t* rnd_off,
                                    const uint8_t* headers, const uint64_t* hdr_off,
                                    const uint8_t* ph, const uint64_t* ph_off,
                                    uint8_t* octets_out, uint64_t* oct_off_out, int8_t* status, bbs_job** job_out);
int bbs_proof_gen_wire_keyed_batch(bbs_ctx* ctx, size_t n, const uint32_t* key_index, const uint8_t* signature_octets,
                                   const uint8_t* msg_bytes, const uint64_t* msg_byte_off, const uint64_t* msg_item_off,
                                   const uint64_t* disclosed_idx, const uint64_t* didx_off,
                                   const uint8_t* random_scalars, const uint64_t* rnd_off,
                                   const uint8_t* headers, const uint64_t* hdr_off,
                                   const uint8_t* ph, const uint64_t* ph_off,
                                   uint8_t* octets_out, uint64_t* oct_off_out, int8_t* status);
/* proof_gen under issuer keys that ARRIVE WITH THE JOB: the four keyed proof_gen exports above with the key set of the call --
 * n_keys and pk_octets in front of key_index, as the eight bbs_*verify*_with_keys_* exports take them: the DISTINCT keys of the
 * job as compressed octets, key_index[i] names a key OF THIS CALL.  A context with no public key and no key set serves the
 * call; the registered set is neither read nor changed; the key bytes are copied by the call.
 * The job prepares its keys on the device as its own first work, on its main stream in front of its ingest kernel.  proof_gen
 * meets the key in the domain alone, so these jobs run a DOMAIN-ONLY key stage: one lane per key decodes the string, tests the
 * twist and [r]Q and hashes the domain midstate -- no Miller-loop line table, no workspace, no field inversion.  Per key the job
 * holds the entry, a status byte and, under bbs_ctx_set_keyed_mixed_lengths, (L + 1) prefixes of 368 bytes (counted by
 * bbs_job_device_bytes); the entry has the layout of a registered key's with an empty table.  The keys are prepared with the
 * upload, once: bbs_job_run on the same job gives the same bytes.
 * STATUS RULE: status AND output bytes are, bit for bit, those of the keyed twin (bbs_*proof_gen*_keyed_*) on a context with the
 * same generators, api_id, window bits, switches and random scalars or seeds whose key set was built by
 * bbs_ctx_add_public_keys_octets(pk_octets), given the same key_index and items.  So an index >= n_keys, or a string
 * registration would refuse (BBS_ST_NONCANONICAL, BBS_ST_NOT_ON_CURVE), gives BBS_ST_UNKNOWN_KEY whatever the other checks
 * decided, and no output (zero record, no octet string); the identity encoding is an accepted key.  The line form of the
 * context does not matter: no key is refused for the form of a table proof_gen never reads (the fail-closed case of the verify
 * exports does not exist here).
 * Errors: those of the keyed twin -- BBS_E_ARG for a NULL key_index with n > 0, a NULL status, a wrong number of random
 * scalars; BBS_E_STATE without generators, or with bbs_ctx_set_mixed_lengths_gen on and bbs_ctx_set_keyed_mixed_lengths off --
 * and BBS_E_ARG for a NULL pk_octets with n_keys > 0 or n_keys > 0xFFFFFFF0.  A missing key set is no error here.
 * Composition: both job forms, bbs_ctx_set_keyed_mixed_lengths (per-item counts; the prefixes per (key, length) are hashed by
 * the stage the verify jobs use), bbs_ctx_set_seeded_random_scalars with per-item seeds or a job seed.
 * bbs_job_key_statuses and bbs_job_key_cache_report answer as for the verify jobs.
 * THE JOB-LOCAL KEY CACHE (bbs_ctx_set_job_key_cache) serves these jobs from the same generation as the verify jobs: same
 * lookup, pins, eviction, bypass and counters.  Hits read the slot's midstate and prefixes, waiting on the device for a slot
 * another job is still publishing.  The MISSES of a cached proof_gen job are prepared by the FULL key stage, line table
 * included, not by the domain-only stage: a slot is whole whoever published it, and a later bbs_*verify*_with_keys_* job may hit
 * it.  The uncached path -- cache off, or the job bypassed -- uses the domain-only stage.
 * NOT covered: sign with job-local keys; bbs_issuer, bbs_pool, the C++ wrapper and the Rust shim; preparing a handful of keys
 * on the host; the subgroup test by the curve endomorphism, which would now shorten both key stages. */
int bbs_core_proof_gen_with_keys_submit(bbs_ctx* ctx, size_t n, size_t n_keys, const uint8_t* pk_octets,
                                        const uint32_t* key_index, const uint8_t* signatures,
                                        const uint8_t* messages, const uint64_t* msg_off,
                                        const uint64_t* disclosed_idx, const uint64_t* didx_off,
                                        const uint8_t* random_scalars, const uint64_t* rnd_off,
                                        const uint8_t* headers, const uint64_t* hdr_off,
                                        const uint8_t* ph, const uint64_t* ph_off,
                                        uint8_t* proofs_fixed_out, uint8_t* commitments_out,
                                        uint64_t* commit_off_out, int8_t* status, bbs_job** job_out);
int bbs_core_proof_gen_with_keys_batch(bbs_ctx* ctx, size_t n, size_t n_keys, const uint8_t* pk_octets,
                                       const uint32_t* key_index, const uint8_t* signatures,
                                       const uint8_t* messages, const uint64_t* msg_off,
                                       const uint64_t* disclosed_idx, const uint64_t* didx_off,
                                       const uint8_t* random_scalars, const uint64_t* rnd_off,
                                       const uint8_t* headers, const uint64_t* hdr_off,
                                       const uint8_t* ph, const uint64_t* ph_off,
                                       uint8_t* proofs_fixed_out, uint8_t* commitments_out,
                                       uint64_t* commit_off_out, int8_t* status);
int bbs_proof_gen_wire_with_keys_submit(bbs_ctx* ctx, size_t n, size_t n_keys, const uint8_t* pk_octets,
                                        const uint32_t* key_index, const uint8_t* signature_octets,
                                        const uint8_t* msg_bytes, const uint64_t* msg_byte_off, const uint64_t* msg_item_off,
                                        const uint64_t* disclosed_idx, const uint64_t* didx_off,
                                        const uint8_t* random_scalars, const uint64_t* rnd_off,
                                        const uint8_t* headers, const uint64_t* hdr_off,
                                        const uint8_t* ph, const uint64_t* ph_off,
                                        uint8_t* octets_out, uint64_t* oct_off_out, int8_t* status, bbs_job** job_out);
int bbs_proof_gen_wire_with_keys_batch(bbs_ctx* ctx, size_t n, size_t n_keys, const uint8_t* pk_octets,
                                       const uint32_t* key_index, const uint8_t* signature_octets,
                                       const uint8_t* msg_bytes, const uint64_t* msg_byte_off, const uint64_t* msg_item_off,
                                       const uint64_t* disclosed_idx, const uint64_t* didx_off,
                                       const uint8_t* random_scalars, const uint64_t* rnd_off,
                                       const uint8_t* headers, const uint64_t* hdr_off,
                                       const uint8_t* ph, const uint64_t* ph_off,
                                       uint8_t* octets_out, uint64_t* oct_off_out, int8_t* status);

/* Keyed sign: ONE context signs under MANY issuer secret keys.  The reference takes the key per call (src/sign.rs:63, &self), so
 * per-item keys are its semantics.
 * The SIGNING KEY SET of a context is an immutable device array of canonical secret scalars, 32 bytes per key, indexed exactly
 * like the key set of the keyed verify / proof_gen entry points and tied to it: key k's public half sk_k * BP2 is registered in
 * the key set under the same index k, so one index names the key for sign, verify, proof_gen and proof_verify on the context.
 * Registration: sk32 holds n little-endian scalars (as bbs_ctx_set_secret_key takes them).  key_status[k] is 1, or
 * BBS_ST_NONCANONICAL for a scalar >= r: a refused key still occupies its index, its public entry is a refused entry, its secret
 * row is zero, and every keyed operation gives items naming it BBS_ST_UNKNOWN_KEY.  sk = 0 is accepted: the identity key.  The
 * public halves of the whole call are derived on the device (the path of bbs_sk_to_pk_batch) and registered as
 * bbs_ctx_add_public_keys registers keys; pk_affine_out (n records of 4 field elements) and is_identity_out (n bytes), each may be
 * NULL, receive them -- byte for byte bbs_sk_to_pk_batch's output, zero for a refused key.  Duplicate keys are legal.
 *   bbs_ctx_set_secret_keys replaces BOTH sets (n_keys = 0 clears both).
 *   bbs_ctx_add_secret_keys appends to both; *first_index = the index of the call's first key; n = 0 only reports the size.
 *   bbs_ctx_secret_key_count: the keys of the key set that have a secret half.
 * The set is immutable once built and grows by appending (a new array of exactly n_old + n rows; the old rows are copied on the
 * device); a keyed sign job holds a reference to the set it was created with, so an append, a replace, a flip of
 * bbs_ctx_set_keyed_mixed_lengths or bbs_ctx_set_generators never reaches a job that exists.  On any failure (BBS_E_NOMEM,
 * BBS_E_HIP) both sets stay as they were.  SECRETS: the device array is cleared, and its stream synchronised, before its memory
 * is released, whoever lets go of it last (bbs_ctx_destroy, a job when it is freed, a setter); the array an append replaces is
 * cleared the same way, and so is every host or device copy the library makes during registration.  No entry point returns a
 * secret.  No constant-time claim is made (as for bbs_ctx_set_secret_key).
 * What drops the signing set: bbs_ctx_set_generators (it drops the key set), bbs_ctx_set_public_keys (n_keys = 0 included),
 * bbs_ctx_set_secret_keys, bbs_ctx_destroy.  bbs_ctx_add_public_keys* does NOT: it appends public-only keys and keeps the signing
 * set.  The context's single key (bbs_ctx_set_secret_key) is untouched and not looked at.
 * BBS_E_ARG for a NULL ctx, a NULL first_index, and a NULL sk32 or key_status with n > 0; BBS_E_STATE without generators.
 *
 * Signing: the arguments of bbs_core_sign_* / bbs_sign_wire_* plus key_index (n entries) after n.  For an item whose key_index
 * names an accepted key with a secret half, the status AND the signature bytes (record or octet string) are, bit for bit, what the
 * un-keyed form gives that item alone on a context with the same generators, api_id and window bits and that key set by
 * bbs_ctx_set_secret_key; with bbs_ctx_set_keyed_mixed_lengths on, item i also has its own count l_i <= L and the comparison
 * context is made with generators[0 .. l_i].  An index >= the key set's size or naming a refused key gives BBS_ST_UNKNOWN_KEY;
 * an index naming an accepted key that was registered public-only gives BBS_ST_NO_SECRET_KEY; both override whatever the other
 * checks decided and leave a zero record (an all-zero octet string).  Such items are decided before the scalar stage and never
 * index the secret array or a midstate.
 * BBS_E_STATE without generators; without a signing set (unless bbs_ctx_set_keyed_mixed_lengths is on: then a missing set is the
 * empty set and every item is BBS_ST_UNKNOWN_KEY, whatever the key set holds); and on a context with
 * bbs_ctx_set_mixed_lengths_gen on unless bbs_ctx_set_keyed_mixed_lengths is on too.  BBS_E_ARG for a NULL key_index with n > 0.
 * Both job forms; the _submit forms return ordinary jobs (bbs_job_wait, bbs_jobs_wait_any, bbs_job_fetch_signatures).
 * NOT covered: an _upload form and the octets (non-wire) keyed form; bbs_issuer, bbs_pool, the C++ wrapper and the Rust shim do
 * not route through these. */
int bbs_ctx_set_secret_keys(bbs_ctx* ctx, size_t n_keys, const uint8_t* sk32, int8_t* key_status, uint8_t* pk_affine_out,
                            int8_t* is_identity_out);
int bbs_ctx_add_secret_keys(bbs_ctx* ctx, size_t n, const uint8_t* sk32, int8_t* key_status, uint8_t* pk_affine_out,
                            int8_t* is_identity_out, uint32_t* first_index);
size_t bbs_ctx_secret_key_count(const bbs_ctx* ctx);   /* keys of the key set that have a secret half */
int bbs_core_sign_keyed_submit(bbs_ctx* ctx, size_t n, const uint32_t* key_index, const uint8_t* messages, const uint64_t* msg_off,
                               const uint8_t* headers, const uint64_t* hdr_off, uint8_t* signatures_out, int8_t* status,
                               bbs_job** job_out);
int bbs_core_sign_keyed_batch(bbs_ctx* ctx, size_t n, const uint32_t* key_index, const uint8_t* messages, const uint64_t* msg_off,
                              const uint8_t* headers, const uint64_t* hdr_off, uint8_t* signatures_out, int8_t* status);
int bbs_sign_wire_keyed_submit(bbs_ctx* ctx, size_t n, const uint32_t* key_index, const uint8_t* msg_bytes,
                               const uint64_t* msg_byte_off, const uint64_t* msg_item_off, const uint8_t* headers,
                               const uint64_t* hdr_off, uint8_t* signature_octets_out, int8_t* status, bbs_job** job_out);
int bbs_sign_wire_keyed_batch(bbs_ctx* ctx, size_t n, const uint32_t* key_index, const uint8_t* msg_bytes,
                              const uint64_t* msg_byte_off, const uint64_t* msg_item_off, const uint8_t* headers,
                              const uint64_t* hdr_off, uint8_t* signature_octets_out, int8_t* status);

/* The reference's PUBLIC sign (src/sign.rs:32-60): raw messages in, signature octet strings out (as bbs_sign_octets_*). */
int bbs_sign_wire_submit(bbs_ctx* ctx, size_t n, const uint8_t* msg_bytes, const uint64_t* msg_byte_off,
                         const uint64_t* msg_item_off, const uint8_t* headers, const uint64_t* hdr_off,
                         uint8_t* signature_octets_out, int8_t* status, bbs_job** job_out);
int bbs_sign_wire_batch(bbs_ctx* ctx, size_t n, const uint8_t* msg_bytes, const uint64_t* msg_byte_off,
                        const uint64_t* msg_item_off, const uint8_t* headers, const uint64_t* hdr_off,
                        uint8_t* signature_octets_out, int8_t* status);

/* core_sign (src/sign.rs:63-133); needs bbs_ctx_set_secret_key.
 * signatures_out: n records A || e (status 1 where written). */
int bbs_core_sign_upload(bbs_ctx* ctx, size_t n, const uint8_t* messages, const uint64_t* msg_off,
                         const uint8_t* headers, const uint64_t* hdr_off, bbs_job** job_out);
int bbs_core_sign_batch(bbs_ctx* ctx, size_t n, const uint8_t* messages, const uint64_t* msg_off,
                        const uint8_t* headers, const uint64_t* hdr_off, uint8_t* signatures_out,
                        int8_t* status);
/* asynchronous form: returns with everything enqueued; bbs_job_wait(job) delivers `status` and writes the records into
 * signatures_out (may be NULL); both buffers must stay valid until then.  The inputs may be released on return. */
int bbs_core_sign_submit(bbs_ctx* ctx, size_t n, const uint8_t* messages, const uint64_t* msg_off,
                         const uint8_t* headers, const uint64_t* hdr_off, uint8_t* signatures_out,
                         int8_t* status, bbs_job** job_out);

/* sign to the wire: signature_octets_out receives n strings of fp_bytes + 32 octets, compress(A) || I2OSP(e, 32) (the
 * byte string of src/tests/test_vector.rs:188-191), all zero for an item whose status is not 1; compression on the device. */
int bbs_sign_octets_submit(bbs_ctx* ctx, size_t n, const uint8_t* messages, const uint64_t* msg_off,
                           const uint8_t* headers, const uint64_t* hdr_off, uint8_t* signature_octets_out,
                           int8_t* status, bbs_job** job_out);
int bbs_sign_octets_batch(bbs_ctx* ctx, size_t n, const uint8_t* messages, const uint64_t* msg_off,
                          const uint8_t* headers, const uint64_t* hdr_off, uint8_t* signature_octets_out,
                          int8_t* status);

/* core_proof_gen (src/proof_gen.rs:116-208: proof_init :211-269, proof_challenge_calculate
 * :272-328, proof_finalize :331-365).  random_scalars replaces the draw at :145-149 and must hold
 * 5 + L - R scalars per item (R = number of disclosed indexes BEFORE dedup, as the reference
 * sizes it), else BBS_E_ARG.  Outputs: proofs_fixed_out (same record as above), commitments_out
 * packed with commit_off_out (n+1 entries; capacity sum_i L_i scalars is always enough). */
int bbs_core_proof_gen_upload(bbs_ctx* ctx, size_t n, const uint8_t* signatures,
                              const uint8_t* messages, const uint64_t* msg_off,
                              const uint64_t* disclosed_idx, const uint64_t* didx_off,
                              const uint8_t* random_scalars, const uint64_t* rnd_off,
                              const uint8_t* headers, const uint64_t* hdr_off,
                              const uint8_t* ph, const uint64_t* ph_off, bbs_job** job_out);
int bbs_core_proof_gen_batch(bbs_ctx* ctx, size_t n, const uint8_t* signatures,
                             const uint8_t* messages, const uint64_t* msg_off,
                             const uint64_t* disclosed_idx, const uint64_t* didx_off,
                             const uint8_t* random_scalars, const uint64_t* rnd_off,
                             const uint8_t* headers, const uint64_t* hdr_off,
                             const uint8_t* ph, const uint64_t* ph_off,
                             uint8_t* proofs_fixed_out, uint8_t* commitments_out,
                             uint64_t* commit_off_out, int8_t* status);
/* proof_gen to the wire: the proofs as octet strings (src/tests/test_vector.rs:199-260: three compressed points, e^,
 * r1^, r3^, the m^ of the undisclosed messages, c; scalars 32 bytes big-endian) packed into octets_out, item i at
 * oct_off_out[i] .. oct_off_out[i + 1] (n + 1 byte offsets; an item whose status is not 1 has an empty string).
 * Capacity n x (3 fp_bytes + 32 (4 + L)) is always enough. */
int bbs_proof_gen_octets_submit(bbs_ctx* ctx, size_t n, const uint8_t* signatures,
                                const uint8_t* messages, const uint64_t* msg_off,
                                const uint64_t* disclosed_idx, const uint64_t* didx_off,
                                const uint8_t* random_scalars, const uint64_t* rnd_off,
                                const uint8_t* headers, const uint64_t* hdr_off,
                                const uint8_t* ph, const uint64_t* ph_off,
                                uint8_t* octets_out, uint64_t* oct_off_out, int8_t* status, bbs_job** job_out);
int bbs_proof_gen_octets_batch(bbs_ctx* ctx, size_t n, const uint8_t* signatures,
                               const uint8_t* messages, const uint64_t* msg_off,
                               const uint64_t* disclosed_idx, const uint64_t* didx_off,
                               const uint8_t* random_scalars, const uint64_t* rnd_off,
                               const uint8_t* headers, const uint64_t* hdr_off,
                               const uint8_t* ph, const uint64_t* ph_off,
                               uint8_t* octets_out, uint64_t* oct_off_out, int8_t* status);
/* The reference's PUBLIC proof_gen (src/proof_gen.rs:78-113) for a context's number of messages in one call: signature
 * octet strings and the messages as RAW BYTES in (layout as bbs_proof_verify_wire_submit), proof octet strings out (as
 * bbs_proof_gen_octets_*).  Statuses: what bbs_signature_from_octets gives when it fails, else msg_to_scalars' panic
 * (BBS_ST_PANIC_DST_TOO_LONG), else core_proof_gen's. */
int bbs_proof_gen_wire_submit(bbs_ctx* ctx, size_t n, const uint8_t* signature_octets,
                              const uint8_t* msg_bytes, const uint64_t* msg_byte_off, const uint64_t* msg_item_off,
                              const uint64_t* disclosed_idx, const uint64_t* didx_off,
                              const uint8_t* random_scalars, const uint64_t* rnd_off,
                              const uint8_t* headers, const uint64_t* hdr_off,
                              const uint8_t* ph, const uint64_t* ph_off,
                              uint8_t* octets_out, uint64_t* oct_off_out, int8_t* status, bbs_job** job_out);
int bbs_proof_gen_wire_batch(bbs_ctx* ctx, size_t n, const uint8_t* signature_octets,
                             const uint8_t* msg_bytes, const uint64_t* msg_byte_off, const uint64_t* msg_item_off,
                             const uint64_t* disclosed_idx, const uint64_t* didx_off,
                             const uint8_t* random_scalars, const uint64_t* rnd_off,
                             const uint8_t* headers, const uint64_t* hdr_off,
                             const uint8_t* ph, const uint64_t* ph_off,
                             uint8_t* octets_out, uint64_t* oct_off_out, int8_t* status);
/* asynchronous form, as bbs_core_sign_submit: bbs_job_wait(job) delivers `status` and the three outputs */
int bbs_core_proof_gen_submit(bbs_ctx* ctx, size_t n, const uint8_t* signatures,
                              const uint8_t* messages, const uint64_t* msg_off,
                              const uint64_t* disclosed_idx, const uint64_t* didx_off,
                              const uint8_t* random_scalars, const uint64_t* rnd_off,
                              const uint8_t* headers, const uint64_t* hdr_off,
                              const uint8_t* ph, const uint64_t* ph_off,
                              uint8_t* proofs_fixed_out, uint8_t* commitments_out,
                              uint64_t* commit_off_out, int8_t* status, bbs_job** job_out);

int bbs_job_run(bbs_job* job);                       /* asynchronous */
int bbs_job_wait(bbs_job* job);
/* Completion-order retire for a serving loop that keeps several batches in flight (the reference has no counterpart: its
 * calls are synchronous, src/proof_verify.rs:19-61).  Jobs submitted together do not finish in submission order -- they
 * share the chip.  What completion order buys is measured: it matters where jobs differ in length or belong to different
 * lists (pipelined lists of BASELINE configs[4]: 7.3 -> 4.9 ms per list, an issuer's groups); on a loop of UNIFORM jobs, the
 * headline loop, it changes nothing (1.42 - 1.44 M/s either way, profiles/r04_b_bench_{any,fifo}_*.json: the convoys are
 * made on the GPU).
 * bbs_jobs_wait_any sleeps until ONE of jobs[0 .. n) -- entries may be NULL; jobs that were never run are ignored -- has
 * finished everything enqueued for it, then does what bbs_job_wait does for that job (delivers statuses / records of the
 * submit forms, BBS_E_STATE if an item was left undecided) and stores its position in *index_out; if several have
 * finished, the one that finished first.  The caller then frees or re-runs that job and calls again with the rest.
 * Event-driven: a host function placed on the job's stream behind its last operation wakes the waiter; nothing polls the
 * device.  BBS_E_STATE if no job of the set has been run.  Jobs of different contexts, curves and devices may be mixed.
 * A job whose last bbs_job_run could not be enqueued completely counts as finished WITH AN ERROR: it is handed out at once
 * (*index_out set) and the call -- like bbs_job_wait on it -- returns BBS_E_HIP and delivers nothing (it never blocks a set).
 * bbs_job_poll: 1 if the job has finished everything enqueued for it (bbs_job_wait will not block), 0 if not. */
int bbs_jobs_wait_any(bbs_job* const* jobs, size_t n, size_t* index_out);
int bbs_job_poll(const bbs_job* job);
size_t bbs_job_size(const bbs_job* job);
/* device memory the job holds until bbs_job_free, in bytes (sizing: INTEGRATION.md); batch verification adds its own */
size_t bbs_job_device_bytes(const bbs_job* job);
int bbs_job_fetch_status(bbs_job* job, int8_t* status);
int bbs_job_fetch_signatures(bbs_job* job, uint8_t* signatures_out);
int bbs_job_fetch_proofs(bbs_job* job, uint8_t* proofs_fixed_out, uint8_t* commitments_out,
                         uint64_t* commit_off_out);
void bbs_job_free(bbs_job* job);

/* Run the job `reps` times back to back and time it with HIP events recorded on the context's
 * own stream: total_ms = whole pipeline; kernel_ms[k] = accumulated time of stage k
 * (n_stages_out stages, names via bbs_job_stage_name).  Used by bench.py for the roofline line. */
int bbs_job_run_timed(bbs_job* job, int reps, float* total_ms, float* kernel_ms, int kernel_cap,
                      int* n_stages_out);
const char* bbs_job_stage_name(const bbs_job* job, int stage);
/* Batch verification, after bbs_job_wait: the groups the job formed, the groups whose 16 combined checks all passed in the last
 * run (the verdict flags are read back from the device by this call), and the items that belong to a group.  It tells the
 * combined path from the per-item one.
 *  - keyed (bbs_ctx_set_keyed_batch_verification): one group per issuer key that reached the threshold; the stages of the
 *    combined path are keyed_rlc_prep, keyed_pip_windows, keyed_pip_group_sums, keyed_rlc_pairing and keyed_bv_decide
 *    (bbs_job_stage_name).
 *  - single-key (bbs_ctx_set_batch_verification; verify and proof_verify, both job forms, mixed lengths included): the whole
 *    job is one group, (1, 1 iff all 16 verdicts are 1, n).  Items decided before the pairing step are counted in n but add
 *    nothing to the combination.
 * Zeros for a job without a combination.  BBS_E_ARG for a NULL argument.
 * bbs_job_bv_verdicts: the raw verdict flags behind that report, 1 = the combined check passed: 16 for a single-key job (one
 * per 8-bit window of the coefficients), 16 * groups for a keyed one (entry g * 16 + w).  *n_out = their count, 0 for a job
 * without a combination.  BBS_E_ARG for a NULL argument, and for cap < count (*n_out is still set, nothing is written). */
int bbs_job_bv_report(bbs_job* job, uint32_t* groups, uint32_t* groups_passed, uint32_t* items_in_groups);
int bbs_job_bv_verdicts(bbs_job* job, int8_t* verdicts, size_t cap, size_t* n_out);
/* Throughput form: `njobs` device-resident batches in flight, step k runs on jobs[k % njobs] (every
 * job owns a HIP stream pair, so independent batches overlap on the GPU).  total_ms = first event to
 * the latest last-stage event; kernel_ms[s] = sum over all steps of stage s's own duration. */
int bbs_jobs_run_timed(bbs_job** jobs, int njobs, int steps, float* total_ms, float* kernel_ms,
                       int kernel_cap, int* n_stages_out);

/* Stage timers for the submit / run forms: jobs created after bbs_ctx_set_stage_timing(ctx, 1) record a HIP event pair
 * around every stage of every run, each on the stream the stage is launched on.  bbs_job_stage_times (after
 * bbs_job_wait) reads the LAST run: total_ms = first stage start .. last stage stop, kernel_ms[k] = duration of stage
 * k (names: bbs_job_stage_name).  BBS_E_STATE for a job created without timing or not yet run. */
int bbs_ctx_set_stage_timing(bbs_ctx* ctx, int enabled);
int bbs_job_stage_times(bbs_job* job, float* total_ms, float* kernel_ms, int kernel_cap, int* n_stages_out);

/* ------------------------------------------------------------------------------------------
 * Unit-parity primitives (hash_to_scalar, G1 multi-scalar multiplication, pairing product).
 * ------------------------------------------------------------------------------------------ */
/* hash_to_scalar (src/utils/core_utilities.rs:11-21) of n ragged messages under one dst. */
int bbs_hash_to_scalar_batch(bbs_ctx* ctx, size_t n, const uint8_t* msgs, const uint64_t* msg_off,
                             const uint8_t* dst, size_t dst_len, uint8_t* scalars_out);
/* seeded_random_scalars (src/utils/core_utilities.rs:84-100) of n ragged seeds under one dst: the device body of
 * bbs_ctx_set_seeded_random_scalars on its own.  Item i's seed is seeds[seed_off[i] .. seed_off[i + 1]) and it produces counts[i]
 * scalars, 32 bytes little-endian each, packed in item order: item i's start at scalar sum(counts[0 .. i)).  status[i]: 1,
 * BBS_ST_PANIC_ELL_TOO_BIG (counts[i] > 170) or, looked at second as in the reference, BBS_ST_PANIC_DST_TOO_LONG (dst_len > 255); the scalars of a refused item are
 * zero.  BBS_E_ARG for the call if a count is 0 (the reference divides by zero there). */
int bbs_seeded_random_scalars_batch(bbs_ctx* ctx, size_t n, const uint8_t* seeds, const uint64_t* seed_off, const uint32_t* counts,
                                    const uint8_t* dst, size_t dst_len, uint8_t* scalars_out, int8_t* status);
/* out[i] = sum_k fixed_scalars[i][k] * G_k  +  sum_m var_scalars[i][m] * var_points[i][m]
 * with G = [P1, Q1, H_1..H_L] of the context (n_fixed <= L+2), affine output. */
int bbs_g1_msm_batch(bbs_ctx* ctx, size_t n, const uint8_t* fixed_scalars, size_t n_fixed,
                     const uint8_t* var_points, const uint8_t* var_scalars, size_t n_var,
                     uint8_t* out_affine, int8_t* status);
/* out = sum_i scalars[i] * points[i]: one large variable-base multi-scalar multiplication over n per-item
 * affine points by the bucket (Pippenger) method (the arkworks `VariableBaseMSM` shape; the reference itself
 * only ever sums <= 38 terms per item, src/proof_verify.rs:163-182).  status[i] = 1, or -40 / -41 for an item
 * that is not canonical / not on the curve (it then contributes nothing). */
int bbs_g1_msm_pippenger(bbs_ctx* ctx, size_t n, const uint8_t* points_affine, const uint8_t* scalars,
                         uint8_t* out_affine, int* out_is_identity, int8_t* status);
/* status[i] = ( e(Pa[i], pk) * e(Pb[i], BP2) == 1 ), or BBS_ST_NONCANONICAL for a coordinate >= p, or, looked at second,
 * BBS_ST_NOT_ON_CURVE; bbs_g1_msm_batch decides its scalars and points in the same order. */
int bbs_pairing_product2_is_one_batch(bbs_ctx* ctx, size_t n, const uint8_t* pa_affine,
                                      const uint8_t* pb_affine, int8_t* status);

/* ------------------------------------------------------------------------------------------
 * bbs_issuer: the reference's four PUBLIC functions over batches whose items differ in their number of messages.
 *
 * The reference chooses the generators by the item's own length on every call: create_generators(messages.len() + 1) in
 * sign / verify / proof_gen (src/sign.rs:44-49, src/verify.rs:30-35, src/proof_gen.rs:91-96) and
 * create_generators(proof.commitments.len() + disclosed_indexes.len() + 1) in proof_verify (src/proof_verify.rs:40-43).
 * A bbs_ctx holds the tables of one generator set; a bbs_issuer holds one context per message count it has seen (created
 * on first use: generators by hash-to-curve on the host, window and line tables on the device, window width by
 * bbs_ctx_set_window_bits(ctx, 0) unless bbs_issuer_set_limits says otherwise) and routes the items of a call: grouped by
 * message count, every group through the context's one-call wire form (bbs_*_wire_submit), all groups in flight together,
 * results scattered back into the caller's order.  Arguments as the bbs_*_wire_* functions of the same name.
 *
 * Statuses: exactly those of the wire form under the item's own context -- so BBS_ST_INVALID_MESSAGE_AND_GENERATORS_LENGTH
 * cannot occur (as in the reference's public functions), EXCEPT for an item with more than max_messages messages (default
 * 1024; bbs_issuer_set_limits), which gets that code and is not computed: a table set per length is device memory an
 * untrusted caller must not be able to allocate without bound.  A proof octet string of the wrong shape is
 * BBS_ST_INVALID_ENCODING (its length does not define a message count).
 *
 * Resident contexts are BOUNDED: at most max_contexts (default 64) and max_table_bytes of window tables (default: half of
 * the device memory free when the issuer builds its first context) stay on the device; when a new message count arrives
 * and a bound is reached, idle contexts leave least-recently-used first (a context is idle when no routed list is in
 * flight on it) and are rebuilt if their length comes back.  The message count of a proof is read from the length of an
 * untrusted octet string: the bounds are what keeps a caller who sends one proof of every length from filling the device.
 * If the context of a group cannot be set up -- the device is out of memory even for the narrowest tables, or every
 * resident context is busy at the limit -- the items of THAT group get BBS_ST_NO_RESOURCES and the rest of the call is
 * served.  A new context is built (hash-to-curve on the host, table build on the device) under that context's own lock:
 * calls for other message counts proceed meanwhile.
 *
 * Threads: bbs_issuer_* may be called on one issuer from several threads.  Submissions to the same context are
 * serialised inside (the bbs_ctx contract: one call at a time per context), every routed list owns its jobs.  The
 * configuration calls (set_public_key, set_secret_key, set_modes) are BBS_E_STATE while a routed list is in flight --
 * its jobs read the contexts' keys -- and otherwise take effect for every context, resident or future, at its next use.
 * ------------------------------------------------------------------------------------------ */
typedef struct bbs_issuer bbs_issuer;
int bbs_issuer_create(int curve, int device_id, const uint8_t* api_id, size_t api_id_len, bbs_issuer** out);
void bbs_issuer_destroy(bbs_issuer* issuer);
int bbs_issuer_set_public_key(bbs_issuer* issuer, const uint8_t* pk_affine, int is_identity);
int bbs_issuer_set_secret_key(bbs_issuer* issuer, const uint8_t* sk32);          /* also sets pk = sk * BP2 */
/* max_messages: longest item served; window_bits: 0 = by free device memory, else 4..22 -- for contexts created afterwards */
int bbs_issuer_set_limits(bbs_issuer* issuer, size_t max_messages, int window_bits);
/* resident contexts: at most max_contexts (>= 1) and max_table_bytes (0 = half of the free device memory at the first
 * context) of tables; idle contexts beyond the new bounds leave at once.  bbs_issuer_table_bytes: what is resident now. */
int bbs_issuer_set_budget(bbs_issuer* issuer, size_t max_contexts, size_t max_table_bytes);
size_t bbs_issuer_table_bytes(bbs_issuer* issuer);
/* bbs_ctx_set_latency_mode / _set_batch_verification (seed from the operating system) / _set_points_in_subgroup on every
 * context of the issuer, present and future */
int bbs_issuer_set_modes(bbs_issuer* issuer, int latency_mode, int batch_verification, int points_in_subgroup);
/* the context serving items of `message_count` messages (created if needed), e.g. to warm it up before traffic arrives, or
 * to drive it directly (one call at a time, and not while the issuer routes lists to it or a bbs_issuer_set_* call is made).
 * A context handed out this way is never evicted, and bbs_issuer_set_public_key / _set_secret_key / _set_modes bring it up to
 * the new configuration BEFORE they return (the other contexts pick it up at their next use). */
int bbs_issuer_context(bbs_issuer* issuer, size_t message_count, bbs_ctx** out);
size_t bbs_issuer_context_count(bbs_issuer* issuer);
/* proof_verify (src/proof_verify.rs:19-61); message count of item i = (its proof's commitments) + (its disclosed indexes) */
int bbs_issuer_proof_verify(bbs_issuer* issuer, size_t n, const uint8_t* proof_octets, const uint64_t* oct_off,
                            const uint8_t* msg_bytes, const uint64_t* msg_byte_off, const uint64_t* msg_item_off,
                            const uint64_t* disclosed_idx, const uint64_t* didx_off,
                            const uint8_t* headers, const uint64_t* hdr_off,
                            const uint8_t* ph, const uint64_t* ph_off, int8_t* status);
/* verify (src/verify.rs:18-50), sign (src/sign.rs:32-60), proof_gen (src/proof_gen.rs:78-113); message count of item i =
 * its number of messages.  sign: fp_bytes + 32 octets per item (zeros where status != 1).  proof_gen: octet strings packed
 * in the caller's order, oct_off_out n + 1 byte offsets, octets_out needs sum_i (3 fp_bytes + 32 (4 + messages_i)) bytes. */
int bbs_issuer_verify(bbs_issuer* issuer, size_t n, const uint8_t* signature_octets,
                      const uint8_t* msg_bytes, const uint64_t* msg_byte_off, const uint64_t* msg_item_off,
                      const uint8_t* headers, const uint64_t* hdr_off, int8_t* status);
int bbs_issuer_sign(bbs_issuer* issuer, size_t n, const uint8_t* msg_bytes, const uint64_t* msg_byte_off,
                    const uint64_t* msg_item_off, const uint8_t* headers, const uint64_t* hdr_off,
                    uint8_t* signature_octets_out, int8_t* status);
int bbs_issuer_proof_gen(bbs_issuer* issuer, size_t n, const uint8_t* signature_octets,
                         const uint8_t* msg_bytes, const uint64_t* msg_byte_off, const uint64_t* msg_item_off,
                         const uint64_t* disclosed_idx, const uint64_t* didx_off,
                         const uint8_t* random_scalars, const uint64_t* rnd_off,
                         const uint8_t* headers, const uint64_t* hdr_off,
                         const uint8_t* ph, const uint64_t* ph_off,
                         uint8_t* octets_out, uint64_t* oct_off_out, int8_t* status);

/* The asynchronous forms, for a serving loop that keeps several lists in flight: *_submit packs the groups, submits them and
 * returns; the inputs may be released at once, `status` and the output buffers must stay valid until bbs_issuer_job_wait,
 * which waits for every group and scatters the results into the caller's order (BBS_E_STATE if an item was left undecided).
 * bbs_issuer_job_free releases the job (after waiting for it if that has not happened); every job of an issuer must be freed
 * before bbs_issuer_destroy (it holds the issuer's contexts).  Arguments as the synchronous calls. */
typedef struct bbs_issuer_job bbs_issuer_job;
int bbs_issuer_proof_verify_submit(bbs_issuer* issuer, size_t n, const uint8_t* proof_octets, const uint64_t* oct_off,
                                   const uint8_t* msg_bytes, const uint64_t* msg_byte_off, const uint64_t* msg_item_off,
                                   const uint64_t* disclosed_idx, const uint64_t* didx_off,
                                   const uint8_t* headers, const uint64_t* hdr_off,
                                   const uint8_t* ph, const uint64_t* ph_off, int8_t* status, bbs_issuer_job** job_out);
int bbs_issuer_verify_submit(bbs_issuer* issuer, size_t n, const uint8_t* signature_octets,
                             const uint8_t* msg_bytes, const uint64_t* msg_byte_off, const uint64_t* msg_item_off,
                             const uint8_t* headers, const uint64_t* hdr_off, int8_t* status, bbs_issuer_job** job_out);
int bbs_issuer_sign_submit(bbs_issuer* issuer, size_t n, const uint8_t* msg_bytes, const uint64_t* msg_byte_off,
                           const uint64_t* msg_item_off, const uint8_t* headers, const uint64_t* hdr_off,
                           uint8_t* signature_octets_out, int8_t* status, bbs_issuer_job** job_out);
int bbs_issuer_proof_gen_submit(bbs_issuer* issuer, size_t n, const uint8_t* signature_octets,
                                const uint8_t* msg_bytes, const uint64_t* msg_byte_off, const uint64_t* msg_item_off,
                                const uint64_t* disclosed_idx, const uint64_t* didx_off,
                                const uint8_t* random_scalars, const uint64_t* rnd_off,
                                const uint8_t* headers, const uint64_t* hdr_off,
                                const uint8_t* ph, const uint64_t* ph_off,
                                uint8_t* octets_out, uint64_t* oct_off_out, int8_t* status, bbs_issuer_job** job_out);
int bbs_issuer_job_wait(bbs_issuer_job* job);
void bbs_issuer_job_free(bbs_issuer_job* job);

/* ------------------------------------------------------------------------------------------
 * Host-side setup helpers: once per ciphersuite / key, no GPU involved.
 * ------------------------------------------------------------------------------------------ */
/* create_generators (src/utils/interface_utilities.rs:47-73) with the curve's hash-to-curve backend
 * (:24-44: BLS12-381 simplified SWU + 11-isogeny; BN254 Shallue-van de Woestijne, pinned by P1 of
 * src/constants.rs:39-51); out = count affine G1 points.  The reference recomputes this on
 * every sign / verify / proof_gen / proof_verify call; callers cache it per (api_id, count). */
int bbs_create_generators(int curve, size_t count, const uint8_t* api_id, size_t api_id_len,
                          uint8_t* out_affine);
/* HashToG1::hash_to_g1 (interface_utilities.rs:17-44), BLS12-381. */
int bbs_hash_to_g1(int curve, const uint8_t* msg, size_t msg_len, const uint8_t* dst, size_t dst_len,
                   uint8_t* out_affine);
/* FromOkm (src/utils/utilities_helper.rs:15-40): 48 big-endian bytes reduced mod r, 32 B LE out -- what
 * calculate_random_scalars (src/utils/core_utilities.rs:70-81) applies to 48 random bytes. */
int bbs_scalar_from_okm(int curve, const uint8_t* okm48, uint8_t* scalar_out);
/* SecretKey::key_gen (src/key_gen.rs:46-81): returns 0 or the KeyGenError code. */
int bbs_key_gen(int curve, const uint8_t* key_material, size_t key_material_len, const uint8_t* key_info,
                size_t key_info_len, const uint8_t* key_dst, size_t key_dst_len, uint8_t* sk32_out);
/* key_gen and sk_to_pk (src/key_gen.rs:46-90) for n keys in one call ON THE DEVICE, one lane per key.  The context gives the
 * curve, the device and the stream only: no generators and no key are needed, and its key, key set and tables are not
 * touched.  key_material / key_info: ragged bytes with n + 1 byte offsets each (item i = bytes[off[i] .. off[i + 1]); the
 * offsets need not start at zero); key_info and ki_off may both be NULL when every key_info is empty; one key_dst for the call.
 * status[i]: 1, or what the one-key call returns for item i, decided in its order -- BBS_ST_INVALID_KEY_MATERIAL_LENGTH,
 * BBS_ST_INVALID_KEY_INFO_LENGTH, BBS_ST_PANIC_DST_TOO_LONG (a key_dst of more than 255 bytes: every item that passed the two
 * length checks), BBS_ST_INVALID_SECRET_KEY.  sk32_out: n x 32 bytes LE; pk_affine_out: n records x.c0 || x.c1 || y.c0 ||
 * y.c1 as bbs_ctx_get_public_key gives them; pk_octets_out: n strings as bbs_public_key_to_octets gives them; either or
 * both may be NULL (both NULL: only the secret keys are derived).  Every output of a refused item is zero.  Synchronous.
 * n = 0 is BBS_OK; BBS_E_ARG for a NULL key_material, km_off, sk32_out or status with n > 0; BBS_E_STATE, and zeroed outputs,
 * if an item was left undecided (fail closed).  Device and staging memory that held key material or secret keys is cleared
 * before it is released; the input is const, clearing the caller's copy is the caller's business.  Nothing is claimed about
 * timing side channels. */
int bbs_key_gen_batch(bbs_ctx* ctx, size_t n, const uint8_t* key_material, const uint64_t* km_off,
                      const uint8_t* key_info, const uint64_t* ki_off, const uint8_t* key_dst, size_t key_dst_len,
                      uint8_t* sk32_out, uint8_t* pk_affine_out, uint8_t* pk_octets_out, int8_t* status);
/* sk_to_pk for n secret keys (32 B LE each) by the same device stage.  status[i]: 1, or BBS_ST_NONCANONICAL for a scalar >= r
 * (zero outputs).  sk = 0 gives the identity key (PublicKey::default()): is_identity_out[i] = 1, a zero record and the
 * identity's compressed encoding.  pk_affine_out, is_identity_out, pk_octets_out may be NULL, but not both key outputs.
 * BBS_E_ARG for a NULL sk32 or status with n > 0. */
int bbs_sk_to_pk_batch(bbs_ctx* ctx, size_t n, const uint8_t* sk32, uint8_t* pk_affine_out, int8_t* is_identity_out,
                       uint8_t* pk_octets_out, int8_t* status);

/* ------------------------------------------------------------------------------------------
 * Wire codec (host side).  Octet strings as in the reference's vectors (src/tests/test_vector.rs:
 * 163-260): signature = compress(A) || e, proof = compress(Abar) || compress(Bbar) || compress(D) ||
 * e^ || r1^ || r3^ || m^_1 .. m^_U || c, public key = compress(pk); scalars 32 B big-endian.
 * `*_from_octets` validate: canonical encodings, on curve, prime-order subgroup, and reject an
 * identity point / zero e where the BBS draft does.  Return 0 or a BBS_ST_* code.
 * (The reference derives ark-serialize's CanonicalSerialize/Deserialize for these types --
 * src/sign.rs:18, src/proof_gen.rs:29, src/key_gen.rs:12 -- without ever exercising them.)
 * Order of the codes.  A point: BBS_ST_NONCANONICAL (a missing compression flag; an identity encoding with a value bit or
 * the sign flag set; x >= p after the flag bits are cleared) before BBS_ST_NOT_ON_CURVE (no root; outside the subgroup).
 * A signature: A's code; BBS_ST_INVALID_ENCODING for A = identity; BBS_ST_NONCANONICAL for e >= r; BBS_ST_INVALID_ENCODING
 * for e = 0.  A proof: BBS_ST_INVALID_ENCODING for the shape; then the FIRST of Abar, Bbar, D that fails decides, with its
 * code or, for the identity, BBS_ST_INVALID_ENCODING; then BBS_ST_NONCANONICAL for any of e^, r1^, r3^, m^_j, c >= r.  The
 * batched forms (`*_from_octets_batch`, bbs_*verify_octets_*, bbs_*_wire_*) decide in the same order.
 * ------------------------------------------------------------------------------------------ */
int bbs_signature_to_octets(int curve, const uint8_t* sig_record, uint8_t* out /* fp_bytes + 32 */);
int bbs_signature_from_octets(int curve, const uint8_t* octets, uint8_t* sig_record_out);
int bbs_proof_to_octets(int curve, const uint8_t* proof_fixed, const uint8_t* commitments, size_t n_commitments,
                        uint8_t* out /* 3 * fp_bytes + 32 * (4 + n_commitments) */);
int bbs_proof_from_octets(int curve, const uint8_t* octets, size_t len, uint8_t* proof_fixed_out,
                          uint8_t* commitments_out, size_t commitments_cap, size_t* n_commitments_out);
/* n compressed G1 points (fp_bytes each, the ciphersuite's encoding) -> affine records on the device: square root,
 * on-curve and prime-order-subgroup checks.  code[i]: 0 ok, 1 ok and the identity (record = zeros), BBS_ST_NONCANONICAL
 * malformed / not canonical, BBS_ST_NOT_ON_CURVE not on the curve or outside the subgroup. */
int bbs_g1_decompress_batch(bbs_ctx* ctx, size_t n, const uint8_t* compressed, uint8_t* out_affine, int8_t* code);
/* bbs_signature_from_octets for n signatures (fp_bytes + 32 bytes each) at once, the point work on the device;
 * status[i] = 1 or the code bbs_signature_from_octets returns for item i; records zeroed where status != 1. */
int bbs_signatures_from_octets_batch(bbs_ctx* ctx, size_t n, const uint8_t* octets, uint8_t* sig_records_out, int8_t* status);
/* bbs_proof_to_octets for n proofs at once (host; no field arithmetic: byte order and the sign flag only).  out needs
 * sum_i (3 * fp_bytes + 32 * (4 + U_i)) bytes; out_off: n + 1 byte offsets; status[i] = 1 or BBS_ST_NONCANONICAL. */
int bbs_proofs_to_octets_batch(int curve, size_t n, const uint8_t* proofs_fixed, const uint8_t* commitments,
                               const uint64_t* commit_off, uint8_t* octets_out, uint64_t* oct_off_out, int8_t* status);
/* bbs_proof_from_octets for n proofs at once: octets ragged (oct_off: n + 1 byte offsets); the 3 n points are
 * decompressed and checked (on curve, prime-order subgroup) on the device, scalars on the host.  status[i] = 1 or the
 * code bbs_proof_from_octets returns for item i; proofs_fixed_out: n records (zeros where status != 1);
 * commitments_out / commit_off_out (n + 1 entries): the commitments of every well-formed item, packed. */
int bbs_proofs_from_octets_batch(bbs_ctx* ctx, size_t n, const uint8_t* octets, const uint64_t* oct_off,
                                 uint8_t* proofs_fixed_out, uint8_t* commitments_out, uint64_t* commit_off_out,
                                 int8_t* status);
int bbs_public_key_to_octets(int curve, const uint8_t* pk_affine, int is_identity, uint8_t* out /* 2 * fp_bytes */);
int bbs_public_key_from_octets(int curve, const uint8_t* octets, uint8_t* pk_affine_out, int* is_identity_out);

/* Key registration self-test: the key-set entries of n keys by two implementations; the caller compares the outputs.  Keys as
 * bbs_ctx_add_public_keys takes them, or, when pk_octets is not NULL, as bbs_ctx_add_public_keys_octets does (pk_affine and
 * is_identity are then ignored).  path 0: the host functions, one key at a time; path 1: the device stage, whatever the key
 * count, read back from the device (with a workspace of ~15 KB per key on BLS12-381, released before the call returns).  entries_out: n x bbs_selftest_key_entry_bytes(curve) bytes; status_out: n; pk_affine_out
 * (octet form only, may be NULL): the decoded records.  Needs the generators; does not touch the context's key set. */
int bbs_selftest_key_entries(bbs_ctx* ctx, size_t n, const uint8_t* pk_affine, const int8_t* is_identity,
                             const uint8_t* pk_octets, int path, uint8_t* entries_out, int8_t* status_out,
                             uint8_t* pk_affine_out);
size_t bbs_selftest_key_entry_bytes(int curve);
/* The domain-only key stage of the bbs_*proof_gen*_with_keys_* jobs alone: the entries and statuses of n strings, read back from
 * the device.  The `hash` part and the status are those of bbs_selftest_key_entries for the same string; the table part is that
 * of a key without a table (no lines, the identity flag set, entries zero).  Needs the generators; does not touch the key set. */
int bbs_selftest_key_domain_entries(bbs_ctx* ctx, size_t n, const uint8_t* pk_octets, uint8_t* entries_out, int8_t* status_out);
/* The prefixes per (key, length) of n keys given as octets (bbs_ctx_set_keyed_mixed_lengths), by two implementations; the caller
 * compares the outputs.  path 0: the host functions registration uses; path 1: the device stages a job with a job-local key
 * set runs (the key stage, then one lane per (key, length)).  rows_out: n x (L + 1) x bbs_selftest_hash_ctx_bytes() bytes, rows of
 * a refused key as every row starts out; status_out: n.  Needs the generators; does not touch the context's key set. */
int bbs_selftest_key_len_rows(bbs_ctx* ctx, size_t n, const uint8_t* pk_octets, int path, uint8_t* rows_out, int8_t* status_out);
/* self-test of the job-local key cache: what the cache holds for each of n strings -- the entry (bbs_selftest_key_entry_bytes
 * each), the status and, where the cache holds rows and rows_out is not NULL, the L + 1 prefixes (bbs_selftest_hash_ctx_bytes
 * each); BBS_E_STATE if the cache is off or one of the strings is not resident */
int bbs_selftest_job_key_cache_entries(bbs_ctx* ctx, size_t n, const uint8_t* pk_octets,
                                       uint8_t* entries_out, int8_t* status_out, uint8_t* rows_out /* may be NULL */);
size_t bbs_selftest_hash_ctx_bytes(void);
/* Keyed batch verification self-test: the segmented bucket kernel and the group sums alone (stages keyed_pip_windows and
 * keyed_pip_group_sums).  n affine G1 points (2 * fp_bytes each, canonical LE, zeros = the identity) given in group order,
 * digits[w * n + i] = the 8-bit coefficient of point i in window w (16 windows), and n_groups groups, group g = the points
 * group_first[g] .. group_first[g] + group_count[g] - 1.  out_affine[(g * 16 + w) * 2 * fp_bytes ..] = sum_i digits[w][i] * P_i
 * over group g (zeros = the identity).  The product library runs the device kernel, one workgroup per (window, segment of at
 * most 4096 points); the host twin its plain double-and-add twin.  BBS_E_ARG for a point that is not canonical or not on the
 * curve, or a group that reaches past n.  Needs no generators and no key. */
int bbs_selftest_segmented_sums(bbs_ctx* ctx, size_t n, const uint8_t* points_affine, const uint8_t* digits /* [16][n] */,
                                size_t n_groups, const uint64_t* group_first, const uint64_t* group_count,
                                uint8_t* out_affine /* [n_groups][16] */);
/* GPU self-test: one Fp12 operation per item (12 Fp values a, b per item, canonical LE, tower order) computed by the
 * one-lane code (on the host) and by the six-lane wavefront-cooperative code; the caller compares the outputs.
 * op: 0 mul, 1..3 Frobenius^k, 4 inverse, 5 conjugate, 6 line multiplication (the point is (b[0], b[1]), any pair of field
 * elements), 7 final exponentiation, 8 square, 10 cyclotomic square, 11 power by the curve parameter (for 10 and 11 the host
 * first maps a into the cyclotomic subgroup: a^((p^6-1)(p^2+1))), 12 is_one (the six-lane comparison with one; out_dist
 * and out_single return the operand).
 * The n items are laid out as the pairing kernels lay theirs out: six lanes per item, ten items per wavefront (item
 * i = wavefront * 10 + group, lanes 60..63 idle), ceil(n / 10) wavefronts, so items 0..9 exercise every group position
 * and n % 10 != 0 a ragged last wavefront.  active (n entries, or NULL = all active): the lanes of an item with active[i] = 0
 * leave before any exchange, as those of a gated item do in the pairing kernels; such an item's out_single, out_dist and
 * flag_out entries are left untouched, and BBS_E_STATE is returned if the device wrote anything for it.
 * line_table / line_index (op 6 only): 0 = the public key's line table (needs a key), 1 = BP2's; the entry, below the
 * table's line count.  out_single: n x 12 Fp, may be NULL; out_dist: n x 12 Fp; flag_out: n entries, 1 for an item whose
 * result the device stored, for op 12 the boolean.  The CPU test build has no six-lane code: BBS_E_ARG. */
int bbs_selftest_f12_batch(bbs_ctx* ctx, int op, size_t n, const uint8_t* a, const uint8_t* b, const int8_t* active,
                           int line_table, int line_index, uint8_t* out_single, uint8_t* out_dist, int8_t* flag_out);
/* The same for one item (ops 0..11) in group 0 of one wavefront, line entry 3 of BP2's table. */
int bbs_selftest_f12(bbs_ctx* ctx, int op, const uint8_t* a, const uint8_t* b, uint8_t* out_single,
                     uint8_t* out_dist);
/* Pairing self-test: the Miller values and the statuses of the latency-form pairing kernels (the two Miller loops of an item
 * on separate wavefronts, then product + final exponentiation), launched unchanged and with the geometry a job gives them,
 * beside the one-lane code run on the host; the caller compares the outputs.  The check is e(Pa, pk) e(+-Pb, BP2) == 1 for
 * the context's public key (BBS_E_STATE without one), in the context's line form (bbs_ctx_set_unit_lines).
 * pa, pb: n affine records each, as bbs_pairing_product2_is_one_batch takes them; negate_b = 1 uses -Pb.  active (n entries,
 * or NULL = all): an item with active[i] = 0 is gated out of every stage and nothing of it is written.
 * miller_in == NULL: on-curve check, both Miller loops, final stage.  status[i] = 1 / 0, or -40 / -41 for a refused item.
 *   miller_dist (may be NULL): for every item that reached the Miller loops, the values of pair 0 = (Pa, pk) and pair
 *   1 = (+-Pb, BP2) as the six-lane kernel left them for the final stage, n x 2 x 12 Fp, canonical LE, tower order;
 *   miller_single (may be NULL): the same two values by the one-lane code.  Rows of inactive and refused items are left as
 *   the caller passed them.  BBS_E_STATE if the device wrote a value or a status for an item that was gated out.
 * miller_in != NULL (n x 2 x 12 Fp, canonical LE, tower order; BBS_E_ARG for a value >= p): no Miller loop; the final stage
 *   alone runs on these values for the active items.  pa / pb are ignored and may be NULL; miller_single and miller_dist
 *   are not written.  The final exponentiation inverts: a pair whose product is zero has no defined status.
 * The CPU test build runs its one-lane stages and fills miller_single only: miller_dist must be NULL there (BBS_E_ARG).
 * n = 0: BBS_OK, nothing written.  A call that returns an error has written nothing. */
int bbs_selftest_pairing_split(bbs_ctx* ctx, size_t n, const uint8_t* pa, const uint8_t* pb, int negate_b,
                               const int8_t* active, const uint8_t* miller_in, uint8_t* miller_single,
                               uint8_t* miller_dist, int8_t* status);
/* Host arithmetic self-test (no GPU): out = sum_k w_k * a_k * b_k in Fp2 computed by the lazily reduced column
 * accumulators the pairing kernel uses (one Montgomery reduction pair per dot product).  a, b: n_terms records
 * c0 || c1 (canonical LE); weights[k] = 1, 2, or 0 for "b_k is its c0 in Fp"; total weight <= 6. */
/* Host arithmetic self-test (no GPU): x^-1 in the base field (scalar_field = 0, fp_bytes LE) or the scalar field
 * (1, 32 bytes LE) by the safegcd inversion the kernels use and by the Fermat power x^(p-2). */
int bbs_selftest_inv(int curve, int scalar_field, const uint8_t* x, uint8_t* out_safegcd, uint8_t* out_fermat);
/* Host arithmetic self-test (no GPU): 3 x0 + 2 x1 (plus = 1) or 3 x0 - 2 x1 (plus = 0) in the base field (fp_bytes LE,
 * canonical in and out) by the single reduction chain with a run-time sign that ends the cyclotomic square. */
int bbs_selftest_lin_pm(int curve, int plus, const uint8_t* x0, const uint8_t* x1, uint8_t* out);
/* Host arithmetic self-test (no GPU): the GLV split of a canonical scalar k (32 bytes LE) as the kernels compute it:
 * k = (+-k1) + (+-k2) * lambda mod r, k1 and k2 below 2^128 (16 bytes LE each), *neg = 1 for a negative half.
 * BLS12-381: lambda = x^2 - 1, k2 = floor(k / lambda), both halves non-negative; BN254: rounding against a short
 * lattice basis (lambda = the cube root of unity whose words are GLV_LAMBDA in params_gen.hpp). */
int bbs_selftest_glv_split(int curve, const uint8_t* k32, uint8_t* k1_16, uint8_t* k2_16, int* neg1, int* neg2);
/* Host arithmetic self-test (no GPU): k0 P0 + k1 P1 + k2 P2 by the joint windowed chain proof_verify uses for T1
 * (src/proof_verify.rs:163-164), plain (glv = 0) or with the GLV split (glv = 1; BLS12-381 points must be in the subgroup).  points: 3 affine records, scalars: 3 x 32 bytes LE canonical. */
int bbs_selftest_mul3(int curve, int glv, const uint8_t* points, const uint8_t* scalars, uint8_t* out_affine);
/* Host arithmetic self-test (no GPU): one half of an Fp4 square as the pairing kernel computes it (four limb-column
 * products, one reduction pair): hi = 0: a^2 + xi b^2, hi = 1: 2 a b, for a, b in Fp2 (c0 || c1, canonical LE);
 * hi | 2 (BLS12-381): the same through the two-pass column accumulators; hi = 1 | 4 (BLS12-381): xi * 2 a b, the
 * form the high lane of the pair (g2, g5) publishes (any other use of bit 4 is BBS_E_ARG). */
int bbs_selftest_fp4sqr(int curve, int hi, const uint8_t* a, const uint8_t* b, uint8_t* out);
int bbs_selftest_f2dot(int curve, size_t n_terms, const uint8_t* a, const uint8_t* b, const uint8_t* weights,
                       uint8_t* out);
/* The same dot product by the two-pass column accumulators (low columns -> Montgomery quotients -> high columns; half the
 * accumulator registers): must equal bbs_selftest_f2dot limb for limb. */
int bbs_selftest_f2dot2(int curve, size_t n_terms, const uint8_t* a, const uint8_t* b, const uint8_t* weights,
                        uint8_t* out);

/* ------------------------------------------------------------------------------------------
 * Pool: core_proof_verify over a LIST of proofs, fanned out over SEVERAL GPUs behind this ABI ("multi-GPU
 * fan-out is internal"; 8(e): split by curve, contiguous ranges per GPU, tables replicated, no data-path collective).
 * The reference verifies one proof per call (src/proof_verify.rs:19-61, core form :64-116); a caller with a list loops over
 * it.  A pool owns one context per (curve, member device) with the same generators and issuer key on every member; a list
 * is handed over as one section per curve in the layout of bbs_core_proof_verify_batch.  Every section is cut into
 * contiguous shares of ceil(n / members) items, every share into jobs of at most max_batch items, and the jobs of a member
 * run from ONE submitting thread per member (owned by the pool) through bbs_core_proof_verify_submit (completion-order
 * retire, curves alternating).  The statuses land in the caller's array in the caller's order: one process drives every GPU, so no
 * exchange between processes exists on this path (the one-process-per-GPU launcher of bench.py exchanges them with one
 * all_gather; both partition by the same rule).  Statuses of every item are exactly those of bbs_core_proof_verify_batch
 * on the item's own curve.
 * ------------------------------------------------------------------------------------------ */
typedef struct bbs_pool bbs_pool;
typedef struct bbs_pv_list {      /* the items of ONE curve of a list, as for bbs_core_proof_verify_batch */
    int curve;
    size_t n;
    const uint8_t* proofs_fixed;
    const uint8_t* commitments;    const uint64_t* commit_off;
    const uint8_t* disclosed_msgs; const uint64_t* dmsg_off;
    const uint64_t* disclosed_idx; const uint64_t* didx_off;
    const uint8_t* headers;        const uint64_t* hdr_off;     /* hdr_off / ph_off may be NULL: all empty */
    const uint8_t* ph;             const uint64_t* ph_off;
    const uint64_t* global_index;  /* NULL: status[k] is item k of this section.  Else: item k is item global_index[k] of
                                    * the caller's whole (mixed) list and its status is written to status[global_index[k]] */
    int8_t* status;
} bbs_pv_list;
/* device_ids: the member devices, in share order; an id may repeat (two context sets on one GPU -- what a test on a
 * one-GPU box uses).  BBS_E_NO_DEVICE if an id does not exist. */
int bbs_pool_create(const int* device_ids, size_t n_devices, bbs_pool** out);
void bbs_pool_destroy(bbs_pool* pool);
size_t bbs_pool_device_count(const bbs_pool* pool);
/* the same configuration on every member's context of `curve` (contexts are created at the first call naming the curve) */
int bbs_pool_set_window_bits(bbs_pool* pool, int curve, int bits);
int bbs_pool_set_generators(bbs_pool* pool, int curve, const uint8_t* generators, size_t count, const uint8_t* api_id,
                            size_t api_id_len);
int bbs_pool_set_public_key(bbs_pool* pool, int curve, const uint8_t* pk_affine, int is_identity);
/* jobs outstanding per member (default 6, the plateau of the single-GPU serving loop) */
int bbs_pool_set_inflight(bbs_pool* pool, int jobs_per_member);
/* member `member`'s context of `curve`, e.g. to run any other operation of this ABI on that device */
int bbs_pool_context(bbs_pool* pool, int curve, size_t member, bbs_ctx** out);
/* Verify a list: the sections are cut into jobs and queued to the members' submitting threads (one per member, inside the
 * library); the call returns at once.  bbs_pool_job_wait blocks until every status of THIS list has been written and returns
 * the first failure of any member (BBS_OK otherwise); then bbs_pool_job_free.  Several lists may be in flight: a member does
 * not drain between lists -- the jobs of the next one go in while the last jobs of this one finish -- and lists complete in
 * submission order per member.  The caller's input buffers AND the bbs_pv_list array's contents must stay valid until
 * bbs_pool_job_wait has returned (unlike bbs_core_proof_verify_submit, the jobs are staged later, by the members' threads).
 * max_batch = 0: 4096.  BBS_E_STATE if a section's curve has no generators / public key yet; BBS_E_ARG before anything is
 * queued if a section is malformed.  The bbs_pool_set_* calls are BBS_E_STATE while a list is in flight.  Free every job
 * before bbs_pool_destroy. */
typedef struct bbs_pool_job bbs_pool_job;
int bbs_pool_proof_verify_submit(bbs_pool* pool, const bbs_pv_list* lists, size_t n_lists, size_t max_batch,
                                 bbs_pool_job** job_out);
int bbs_pool_job_wait(bbs_pool_job* job);
void bbs_pool_job_free(bbs_pool_job* job);
/* submit + wait + free */
int bbs_pool_proof_verify(bbs_pool* pool, const bbs_pv_list* lists, size_t n_lists, size_t max_batch);

#ifdef __cplusplus
}
#endif
#endif /* BBS_SIGN_AMD_H */
