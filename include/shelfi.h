/*
 * shelfi.h — C ABI of the MI355X-native CKKS weighted-average aggregator.
 *
 * Drop-in replacement for the compute behind the reference's pybind11 module
 * SHELFI_FHE (palisade_pybind/SHELFI_FHE/src/binding.cpp:14-31, class CKKS in
 * include/ckks.h:27-54 implementing Scheme in include/scheme.h:15-32).  Each
 * entry point below names the reference method it replaces.  Plain C: opaque
 * context, raw pointers and sizes, int status codes (0 = OK), a thread-local
 * message via shelfi_last_error().  Caller-owned inputs are never retained;
 * library-owned outputs are released with shelfi_free().
 *
 * All arithmetic runs in hand-written HIP kernels on an AMD Instinct MI355X
 * (gfx950).  There is no CPU compute path: on a host without a usable gfx950
 * device, shelfi_ctx_create() fails with SHELFI_ERR_DEVICE.
 */
#ifndef SHELFI_H_
#define SHELFI_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SHELFI_ABI_VERSION 1

/* status codes */
#define SHELFI_OK 0
#define SHELFI_ERR_ARG -1      /* bad argument (maps to ValueError) */
#define SHELFI_ERR_DEVICE -2   /* HIP / device failure (RuntimeError) */
#define SHELFI_ERR_IO -3       /* file read/write failure */
#define SHELFI_ERR_FORMAT -4   /* malformed / mismatched ciphertext or key blob */
#define SHELFI_ERR_STATE -5    /* keys not loaded, etc. */
#define SHELFI_ERR_RANGE -6    /* value outside the CKKS encoding/decoding range */
#define SHELFI_ERR_PRECISION -7 /* decode: approximation error too high (PALISADE math_error) */

typedef struct shelfi_ctx shelfi_ctx;

/* Parameters of a context (filled by shelfi_ctx_info). */
typedef struct shelfi_info {
  uint32_t ring_dim;       /* N */
  uint32_t num_towers;     /* L = multDepth + 1 */
  uint32_t batch;          /* slots per ciphertext (ckks.h:31 batchSize) */
  uint32_t scale_bits;     /* ckks.h:32 scaleFactorBits */
  uint32_t first_mod_bits; /* bits of q_0 */
  int32_t device;          /* HIP device ordinal */
  uint64_t moduli[16];     /* q_0 .. q_{L-1} */
  uint64_t roots[16];      /* minimal primitive 2N-th roots psi_t */
  double delta;            /* level-0 scaling factor = (double)q_{L-1} (EXACTRESCALE) */
  uint64_t key_id;         /* 0 until keys are loaded/generated */
  int32_t keys_loaded;
  int32_t palisade_keys;   /* 1 if the keys came from PALISADE-format files */
  uint32_t slot_packing;   /* SHELFI_PACK_REAL or SHELFI_PACK_COMPLEX (shelfi_set_slot_packing) */
  uint32_t values_per_ct;  /* V: doubles one ciphertext carries, batch or 2 * batch */
} shelfi_info;

/* ---- library ------------------------------------------------------------ */
int shelfi_abi_version(void);
/* Re-read the SHELFI_* A/B probe switches from the environment.  They are read
 * when a context is created and here, never by a launch; call between calls, not during one. */
void shelfi_reload_switches(void);
const char* shelfi_last_error(void);
void shelfi_free(void* p);

/* Host-only parameter generation (no device needed): PALISADE ParamsGen rule for
 * EXACTRESCALE chains, as called by ckks.cpp:28 genCryptoContextCKKS(multDepth,
 * scaleFactorBits, batchSize).  ring_dim = 0 picks the PALISADE ring dimension
 * (HE-standard 128-bit classic, N >= 2*batch).  Writes L moduli and roots. */
int shelfi_params_generate(uint32_t ring_dim, uint32_t num_towers, uint32_t scale_bits,
                           uint32_t first_mod_bits, uint32_t batch, uint32_t* ring_dim_out,
                           uint64_t* moduli_out, uint64_t* roots_out);

/* Host-only PALISADE reader (no device needed): parses a reference cryptodir
 * (cryptocontext.txt / key-public.txt / key-private.txt, ckks.cpp:11-23).  Call with
 * q/psi/pk/sk = NULL to query N and L first; q/psi hold 16 entries, pk 2*L*N, sk L*N. */
int shelfi_read_palisade(const char* cryptodir, uint32_t* ring_dim, uint32_t* num_towers,
                         uint64_t* moduli, uint64_t* roots, uint64_t* pk, uint64_t* sk);

/* ---- context lifecycle (ckks.cpp:5-9 CKKS::CKKS) -------------------------- */
/* num_towers = multDepth + 1 (reference: multDepth = 1, ckks.cpp:26). */
int shelfi_ctx_create(uint32_t ring_dim, uint32_t num_towers, uint32_t scale_bits,
                      uint32_t first_mod_bits, uint32_t batch, int device, shelfi_ctx** out);
void shelfi_ctx_destroy(shelfi_ctx* ctx);
int shelfi_ctx_info(const shelfi_ctx* ctx, shelfi_info* out);
/* Deterministic ("parity") mode: encryption/keygen randomness derived from `seed`
 * (ChaCha20 stream spec in DESIGN.md).  seed = 0 restores OS-entropy seeding. */
int shelfi_set_seed(shelfi_ctx* ctx, uint64_t seed);

/* ---- keys ----------------------------------------------------------------- */
/* ckks.cpp:25-59 genCryptoContextAndKeyGen: generates keys on the device and writes
 * cryptodir/{cryptocontext,key-public,key-private}.txt in PALISADE 1.11's cereal
 * PortableBinary format (ckks.cpp:41-55; byte-identical to what the reference writes for
 * the same parameters, keys and key tag).  cryptodir = "" or NULL: keys stay in memory. */
int shelfi_keygen(shelfi_ctx* ctx, const char* cryptodir);
/* ckks.cpp:11-23 loadCryptoParams: reads PALISADE 1.11 cereal-binary files (the
 * reference's code/resources/cryptoparams/, or shelfi_keygen's) and this library's
 * round-1 key files ("SHCC"/"SHPK"/"SHSK"). */
int shelfi_load(shelfi_ctx* ctx, const char* cryptodir);
/* Raw key import/export ([2][L][N] public (b, a), [L][N] secret, EVALUATION). */
int shelfi_set_keys(shelfi_ctx* ctx, const uint64_t* pk, const uint64_t* sk);
int shelfi_get_keys(const shelfi_ctx* ctx, uint64_t* pk, uint64_t* sk);

/* ---- bytes API (binding.cpp:26-31) ---------------------------------------- */
/* ckks.cpp:61-104 encrypt: n doubles -> blob of ceil(n/batch) ciphertexts. */
int shelfi_encrypt(shelfi_ctx* ctx, const double* x, size_t n, uint8_t** out, size_t* out_len);
/* Same into a caller-owned buffer (out = NULL: only *out_len); H2D, kernels and D2H
 * are pipelined over ciphertext chunks. */
int shelfi_encrypt_into(shelfi_ctx* ctx, const double* x, size_t n, uint8_t* out, size_t out_cap,
                        size_t* out_len);
/* ckks.cpp:264-320 computeWeightedAverage: C blobs, float32 weights (ckks.cpp:287). */
int shelfi_weighted_average(shelfi_ctx* ctx, const uint8_t* const* blobs, const size_t* lens,
                            const float* weights, size_t num_learners, uint8_t** out,
                            size_t* out_len);
/* Same, writing into a caller-owned buffer (out = NULL: only *out_len = result size).
 * Copies, aggregation and the copy-out are pipelined over ciphertext chunks. */
int shelfi_weighted_average_into(shelfi_ctx* ctx, const uint8_t* const* blobs, const size_t* lens,
                                 const float* weights, size_t num_learners, uint8_t* out,
                                 size_t out_cap, size_t* out_len);
/* ckks.cpp:170-213 decrypt: blob -> n doubles (caller-owned out[n]). */
int shelfi_decrypt(shelfi_ctx* ctx, const uint8_t* blob, size_t len, size_t n, double* out);

/* Decode noise flooding, PALISADE 1.11 CKKSPackedEncoding::Decode:
 * symmetrize, estimate sigma from the anti-symmetric part, add Gaussian noise of
 * stddev sqrt(m_factor + 1) * max(sigma, sqrt(N)/8) (m_factor = CKKS_M_FACTOR, 1 in
 * PALISADE), fail with SHELFI_ERR_PRECISION when log2 sigma > scale_bits - 5.  ON by
 * default with m_factor 1, like the Decrypt it replaces (ckks.cpp:189); enabled = 0 gives
 * the exact, deterministic decode (parity mode).  Applies to shelfi_decrypt and
 * shelfi_dev_decrypt.  Randomness: the ctx's seeded / OS-random ChaCha20 stream. */
int shelfi_set_decode_noise(shelfi_ctx* ctx, int enabled, double m_factor);
/* Decode range (round 6).  exact = 0 (default): decrypt reads the shortest tower prefix whose
 * modulus Q' exceeds 2^130 and reconstructs each coefficient exactly while its centred value is in
 * [-2^127, 2^127); a coefficient outside that range is detected and the call is redone over every
 * tower through an exact multi-word CRT, up to (Q - 1) / 2 (PALISADE's BigInteger decode,
 * ckks.cpp:189).  A chain at or below 2^130 (multDepth = 1, or a ciphertext of one or two towers at
 * a lower level) is decoded whole: there the fast pass is sure of a coefficient only while
 * |X| < Q/2 - Q 2^-16, and any coefficient nearer to +-Q/2 sends the call to the exact pass, so
 * decrypt is exact up to (Q - 1) / 2 on such chains too.  On longer chains the prefix cannot see a
 * value of |X| >= Q'/2 whose residue mod Q' falls inside [-2^127, 2^127) (|X| >= 2^163 at
 * 2^15 / L4): that alone is wrong by default.  exact = 1: every decrypt reads every tower and
 * decodes through the exact CRT (same output bits wherever both are defined; ~25% slower at
 * 2^15 / L4).  Applies to shelfi_decrypt and the shelfi_dev_decrypt* calls. */
int shelfi_set_decode_exact(shelfi_ctx* ctx, int exact);
/* Decrypt calls of this context (shelfi_decrypt, shelfi_dev_decrypt*) whose fast pass met a
 * coefficient outside its range and were redone through the exact CRT.  Calls made under
 * shelfi_set_decode_exact(ctx, 1) have no fast pass and do not count. */
int shelfi_decode_redo_count(shelfi_ctx* ctx, uint64_t* count);
/* Encrypt calls of this context (shelfi_encrypt*, shelfi_dev_encrypt) whose fast pass met a message
 * coefficient above 2^61 in magnitude and were redone on the large-value path (PALISADE's
 * approxFactor scale-down).  One per call, however many of its ciphertexts or chunks were flagged; a
 * call refused for a non-finite value does not count. */
int shelfi_encode_redo_count(shelfi_ctx* ctx, uint64_t* count);
/* logError of the last flooded decrypt (max over its ciphertexts; PALISADE
 * Plaintext::GetLogError), -1 if none.  Precision = scale_bits - logError. */
int shelfi_decode_log_error(shelfi_ctx* ctx, int* log_error);

/* Blob inspection: number of ciphertexts, depth, scale, key id. */
int shelfi_blob_info(const uint8_t* blob, size_t len, uint64_t* num_cts, uint32_t* depth,
                     double* scale, uint64_t* key_id);
/* Beside shelfi_blob_info (what a receiver reads before the Deserial of ckks.cpp:281): the blob's version --
 * 1 uint64 residues, 2 packed, 3 seeded (shelfi_set_wire_format's 0, 2 and 3).  Header and length are checked
 * as shelfi_blob_info checks them. */
int shelfi_blob_version(const uint8_t* blob, size_t len, uint32_t* version);
/* Build a blob from raw residues [K][2][L][N] (host) with the given metadata. */
int shelfi_blob_pack(const shelfi_ctx* ctx, const uint64_t* residues, uint64_t num_cts,
                     uint32_t depth, double scale, uint8_t** out, size_t* out_len);
/* Offset of the residue payload inside a blob (64-byte header). */
size_t shelfi_blob_header_bytes(void);
/* Host-only: a blob's residues as [K][2][L][N] uint64 (out: K*2*L*N words) — a version-1 payload
 * copied, a version-2 (packed wire, shelfi_set_wire_format 2) payload unpacked.  A version-3 (seeded)
 * blob is refused (SHELFI_ERR_ARG): its c1 is a ChaCha20 stream, expanded on the device by
 * shelfi_dev_blob_unpack. */
int shelfi_blob_unpack(const shelfi_ctx* ctx, const uint8_t* blob, size_t len, uint64_t* out);

/* ---- PALISADE 1.11 wire format -------------- */
/* The reference's bytes are cereal PortableBinary archives of
 * vector<Ciphertext<DCRTPoly>> (ckks.cpp:98-100, :281, :308-310).  With keys loaded from
 * the reference's PALISADE files, shelfi_set_wire_format(ctx, 1) makes encrypt produce
 * such archives; computeWeightedAverage and decrypt accept archives and blobs alike,
 * and computeWeightedAverage answers in its inputs' format. */
typedef struct {
  uint32_t ring_dim, num_towers;
  uint64_t num_cts;
  uint64_t moduli[16];
  uint64_t depth, level;
  double scale;
  uint32_t encoding;      /* 4 = CKKSPacked */
  int32_t vector_archive; /* 0: a single Ciphertext (e.g. mkhe's CT1.txt) */
  uint64_t ctx_offset, ctx_length; /* the embedded context object inside the archive */
  char keytag[257];
} shelfi_palisade_info;
/* 0 blob (the C ABI's default), 1 PALISADE archive (the Python / C++ front ends' default once keys
 * are generated or loaded in PALISADE's files, as ckks.cpp:98-103 writes them), 2 packed blob
 * (version 2: the residues at their moduli's widths, the arena's slice format with C = 1 — 218 of
 * 256 bits per coefficient at 2^15/L4, so a PCIe-bound upload carries 15% fewer bytes; DESIGN.md
 * §5.3), 3 seeded blob (version 3, DESIGN.md §2.17: beside cc->Encrypt (ckks.cpp:81), for learners that
 * hold the secret key as the reference's do -- encrypt is symmetric, c1 = a is expanded from a 32-byte
 * public seed by whoever reads the blob, and only c0 travels, packed: 892,928 bytes a ciphertext at
 * 2^15/L4 where the packed blob has 1,785,856.  The blob is the 64-byte header, the seed, 32 zero bytes,
 * then one packed group (c0) a ciphertext.  encrypt then needs the whole secret key: SHELFI_ERR_STATE on
 * a context whose secret is a threshold share (shelfi_multiparty_keygen), SHELFI_ERR_RANGE for a
 * coefficient above 2^61 (no large-value path).  The seed is public; two encryptions under one (seed,
 * ciphertext index) leak the difference of their messages, so a seed is drawn per call).  Every entry
 * that takes ciphertext bytes accepts all four; computeWeightedAverage answers seeded inputs (all learners
 * seeded, or none) in format 2: a sum of seeded ciphertexts is not seeded. */
int shelfi_set_wire_format(shelfi_ctx* ctx, int format);
/* The format encrypt answers in right now (0 .. 3; -1 for a NULL context). */
int shelfi_get_wire_format(const shelfi_ctx* ctx);
/* Slot packing, context state like the wire format.  SHELFI_PACK_REAL (the default): one
 * double per slot, the slot's imaginary half unused, as the reference encodes.  SHELFI_PACK_COMPLEX: slot s of
 * ciphertext k holds x[k V + 2 s] + i x[k V + 2 s + 1], V = 2 * batch values a ciphertext (shelfi_info's
 * values_per_ct), so every call that takes or returns n doubles uses ceil(n / V) ciphertexts: shelfi_encrypt(_into),
 * shelfi_decrypt, shelfi_fuse_decrypt, shelfi_dev_encrypt(_seeded), shelfi_dev_encode, shelfi_dev_decrypt(_level,
 * _sum) and shelfi_dev_fuse_decrypt.  Values at or beyond n encode as 0; decrypt returns the first n.  The device
 * calls then need x_dev / out_dev 16-byte aligned.  Everything between the two ends (the weighted average, the
 * arena, the wire formats, partial decryption) is linear with real weights and runs unchanged; slot products are
 * complex products (a norm is dot(u, conjugate(u)), shelfi_dev_conjugate).  Decode noise flooding estimates its
 * sigma from the imaginary parts and cannot run on complex slots: with it enabled (the default) a complex-mode
 * decrypt or fusion fails with SHELFI_ERR_STATE before anything runs -- turn it off with
 * shelfi_set_decode_noise(ctx, 0, 1.0).  The mode is not recorded in a ciphertext: both ends must agree on it.
 * An unknown mode: SHELFI_ERR_ARG. */
#define SHELFI_PACK_REAL 0
#define SHELFI_PACK_COMPLEX 1
int shelfi_set_slot_packing(shelfi_ctx* ctx, int mode);
/* The mode in force (-1 for a NULL context). */
int shelfi_get_slot_packing(const shelfi_ctx* ctx);
/* Host-only: parse an archive; residues [K][2][L][N] copied out when non-NULL. */
int shelfi_palisade_parse(const uint8_t* archive, size_t len, shelfi_palisade_info* info,
                          uint64_t* residues);
/* Host-only: write an archive (free with shelfi_free) from residues [K][2][L][N] and an
 * embedded context object (shared-pointer ids from 3: shelfi_palisade_key_context).
 * flags: SHELFI_PAL_VECTOR = vector<Ciphertext> (else a single Ciphertext, K = 1);
 * SHELFI_PAL_KEY_PARAMS = the polynomials carry the key's own parameter objects, as in
 * every archive the reference's encrypt / computeWeightedAverage writes (its keys are
 * loaded from files); without it they reference the context's (CT1.txt). */
#define SHELFI_PAL_VECTOR 1
#define SHELFI_PAL_KEY_PARAMS 2
int shelfi_palisade_write(const uint8_t* ctx_obj, size_t ctx_len, const char* keytag,
                          uint32_t ring_dim, uint32_t num_towers, const uint64_t* moduli,
                          uint64_t num_cts, const uint64_t* residues, uint64_t depth, uint64_t level,
                          double scale, int flags, uint8_t** out, size_t* out_len);
/* Host-only: cryptocontext.txt as ckks.cpp:41 serializes the context of
 * genCryptoContextCKKS(multDepth = L - 1, scale_bits, batch) with these towers. */
int shelfi_palisade_context_file(uint32_t ring_dim, uint32_t num_towers, const uint64_t* moduli,
                                 const uint64_t* roots, uint32_t scale_bits, uint32_t batch,
                                 uint8_t** out, size_t* out_len);
/* Host-only: key-public.txt (is_public = 1, polys [2][L][N]: b, a) or key-private.txt
 * (polys [L][N]: s) around an embedded context object (ids from 3), ckks.cpp:48,53. */
int shelfi_palisade_key_file(const uint8_t* ctx_obj, size_t ctx_len, const char* keytag,
                             const uint64_t* polys, int is_public, uint8_t** out, size_t* out_len);
/* Host-only: the embedded context object (free with shelfi_free) and key tag of a
 * PALISADE key-public.txt (ckks.cpp:48). */
int shelfi_palisade_key_context(const uint8_t* pub, size_t len, uint8_t** ctx_obj, size_t* ctx_len,
                                char keytag[257]);
/* Host-only: a cryptocontext.txt's context object re-embedded one shared-pointer id
 * later (what key and ciphertext archives hold). */
int shelfi_palisade_embed_context(const uint8_t* ctxfile, size_t len, uint8_t** out,
                                  size_t* out_len);

/* ---- device-resident batch API (HBM in, HBM out; `stream` = hipStream_t) ---- */
/* Ciphertext batches are [K][2][L][N] uint64 in HBM (same order as the blob
 * payload).  Work is enqueued on `stream` exactly as given (NULL = the legacy
 * default stream, e.g. PyTorch's default stream); wavg/modq/ntt return without
 * syncing, encrypt/decrypt synchronise `stream` before returning (they reuse the
 * context's scratch arena). */

/* sum_c W_c * in[c] mod q_t, W_c = (int64)((double)w[c] * delta + 0.5) (EvalMult +
 * EvalAdd, ckks.cpp:286-297).  in_dev: host array of C device pointers. */
int shelfi_dev_wavg(shelfi_ctx* ctx, const uint64_t* const* in_dev, const float* w, size_t C,
                    size_t K, uint64_t* out_dev, void* stream);
/* Packed learner-interleaved arena: the aggregator's resident layout for C learners' K
 * ciphertexts.  Rows of 512 residues in [K][2][L][N] order; a row holds the C learners'
 * slices side by side, and every residue of tower t is packed to U_t bits (bitlength(q_t) when
 * that is 1 mod 4, else rounded up to a multiple of 4; >= 32): 60/53/52/53 at the reference's
 * 2^15/L4, 218 of 256 bits per coefficient, so one aggregation wave reads one contiguous C-slice
 * region and the launch moves 14% fewer bytes
 * (DESIGN.md §3).  The layout is opaque: size it with shelfi_arena_words() (uint64 words;
 * ciphertexts [k0, k1) of an arena start at word k0 * shelfi_arena_words(ctx, C, 1) and are
 * themselves an arena of k1 - k0 ciphertexts).  shelfi_dev_arena_put packs learner
 * `learner`'s [K][2][L][N] uint64 batch (device memory, or host memory if src_on_host) into
 * its slices. */
size_t shelfi_arena_words(const shelfi_ctx* ctx, size_t C, size_t K);
/* Every put validates what landed: one device pass over the learner's slices checks that
 * each residue is < q_t (the aggregation's carry-free limb sums assume canonical
 * residues), and the call returns after it (synchronises `stream`).  A refused slot
 * (SHELFI_ERR_FORMAT) stays marked: shelfi_dev_wavg_arena over a range of that arena
 * fails with SHELFI_ERR_STATE until a valid put replaces the slot. */
int shelfi_dev_arena_put(shelfi_ctx* ctx, const void* src, int src_on_host, size_t K, size_t learner,
                         size_t C, uint64_t* arena_dev, void* stream);
/* A learner's upload as it arrives over the wire — a library blob or a PALISADE archive
 * (ckks.cpp:276-281's per-learner bytes) — placed into its arena slot.  The header is
 * checked against the context before any byte is copied: ring dimension, towers and
 * moduli (params_id), the key (key_id / PALISADE keyTag, as EvalAdd refuses other keys,
 * SURVEY App. B.7), the CKKS-packed encoding and the length; the batch must hold exactly
 * K ciphertexts.  Refusals are SHELFI_ERR_FORMAT; the residues are then validated as
 * for shelfi_dev_arena_put.  A refused header marks the slot refused as well (its previous
 * contents are not aggregated as if the upload had landed). */
int shelfi_dev_arena_put_blob(shelfi_ctx* ctx, const uint8_t* blob, size_t len, size_t K, size_t learner,
                              size_t C, uint64_t* arena_dev, void* stream);
/* Forget the refusal marks of an arena's memory [arena_dev, arena_dev + words) before it is
 * freed or reused (no reference counterpart: the reference has no resident arena).  A put
 * into a differently shaped arena over the same memory, and a parameter or key reload, drop
 * stale marks by themselves. */
int shelfi_dev_arena_release(shelfi_ctx* ctx, const uint64_t* arena_dev, size_t words);
/* Host-synchronous check that every residue of a [K][2][L][N] device batch is < q_t
 * (SHELFI_ERR_FORMAT otherwise): the upload check of SHELFI_FHE.device.Arena's uint64 layout, which
 * small launches aggregate with shelfi_dev_wavg (the packed arena checks while packing). */
int shelfi_dev_check_residues(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, void* stream);
/* shelfi_dev_wavg over an arena of C learners (same arithmetic and result). */
int shelfi_dev_wavg_arena(shelfi_ctx* ctx, const uint64_t* arena_dev, const float* w, size_t C,
                          size_t K, uint64_t* out_dev, void* stream);
/* The same aggregation written packed: K ciphertexts in the arena's slice format with C = 1
 * (shelfi_arena_words(ctx, 1, K) uint64 words at out_packed), the packed exchange's send form. */
int shelfi_dev_wavg_arena_packed(shelfi_ctx* ctx, const uint64_t* arena_dev, const float* w, size_t C,
                                 size_t K, uint64_t* out_packed, void* stream);
/* sum_g x_g mod q_t of G <= 16 packed (C = 1) batches of K ciphertexts stacked stride_words uint64
 * words apart (>= shelfi_arena_words(ctx, 1, K)) -> out_dev [K][2][L][N], canonical residues: the
 * packed exchange's receive side (EvalAdd of the ranks' partial aggregates). */
int shelfi_dev_sum_packed(shelfi_ctx* ctx, const uint64_t* stacked, size_t G, size_t K, size_t stride_words,
                          uint64_t* out_dev, void* stream);
/* Output placement for a resident arena (no reference counterpart: a property of where
 * the aggregate lands in HBM).  The arena launch's time depends on the physical
 * placement of its output buffer relative to the arena (up to 12%,
 * reproducible per buffer pair).  Runs shelfi_dev_wavg_arena into each of the n
 * candidate [K][2][L][N] buffers (1 warm-up + `launches` timed launches each, HIP
 * events on `stream`), writes each one's mean launch time to ms[i] (if ms), and the
 * index of the fastest to *best.  Every candidate ends up holding the aggregate. */
int shelfi_dev_wavg_arena_pick_output(shelfi_ctx* ctx, const uint64_t* arena_dev, const float* w,
                                      size_t C, size_t K, uint64_t* const* candidates, size_t n,
                                      int launches, size_t* best, float* ms, void* stream);
/* Folds a collective's uint64 SUM of G <= 15 reduced partial sums back into [0, q_t)
 * (multi-GPU combine: local shelfi_dev_wavg -> RCCL reduce/reduce_scatter -> this). */
int shelfi_dev_modq(shelfi_ctx* ctx, uint64_t* buf_dev, size_t K, void* stream);
/* ---- multi-GPU combine over RCCL (one process per GPU, SURVEY §8 e) --------
 * Each rank aggregates its own learners with shelfi_dev_wavg / _arena into a partial
 * of K ciphertexts; these calls combine the partials exactly (uint64 SUM over <= 16
 * ranks, then the mod-q fold of shelfi_dev_modq), bit-identical to aggregating every
 * learner on one GPU.  Collective: every rank of the communicator makes the same call
 * in the same order.  Replaces, for the multi-GPU path, the serial EvalAdd loop of
 * CKKS::computeWeightedAverage (ckks.cpp:291-297). */
#define SHELFI_COMM_ID_BYTES 128
/* rank 0 makes the 128-byte id and hands it to every rank out of band */
int shelfi_comm_unique_id(uint8_t* id_out);
/* bind a communicator of `world` (<= 16) ranks to ctx (its device), replacing any previous one */
int shelfi_comm_init(shelfi_ctx* ctx, const uint8_t* id, int rank, int world);
int shelfi_comm_destroy(shelfi_ctx* ctx);
/* rank/world of ctx's communicator (-1 / 0 if none) */
int shelfi_comm_info(const shelfi_ctx* ctx, int* rank, int* world);
/* in place: the combined aggregate lands on `root` (other ranks' buffers are scratch) */
int shelfi_dev_reduce(shelfi_ctx* ctx, uint64_t* partial_dev, size_t K, int root, void* stream);
/* in place: the combined aggregate on every rank */
int shelfi_dev_allreduce(shelfi_ctx* ctx, uint64_t* partial_dev, size_t K, void* stream);
/* rank r receives ciphertexts [r K/W, (r+1) K/W) of the combined aggregate in out_dev
 * (K % W == 0): each rank then decrypts its own slice, nothing is gathered */
int shelfi_dev_reduce_scatter(shelfi_ctx* ctx, const uint64_t* partial_dev, size_t K,
                              uint64_t* out_dev, void* stream);
/* The whole learner-sharded step in one call, pipelined: this rank's arena of C learners
 * (K ciphertexts each) is aggregated piece by piece on `stream`, and each piece's
 * ncclReduceScatter runs on the context's own comm stream (ordered by HIP events) while the
 * next piece is aggregated.  Rank r receives the combined aggregate of global ciphertexts
 * [r Ks, min(K, (r+1) Ks)), Ks = shelfi_combine_share_cts(ctx, K) = ceil(K / W), contiguous in
 * share_dev (Ks ciphertexts; slots past K are zero).  send_dev is scratch of W * Ks
 * ciphertexts.  fold = 1 folds each piece into [0, q_t) on the comm stream; fold = 0 leaves
 * the uint64 sums of W residues for shelfi_dev_decrypt_sum, which folds them on load (no
 * separate pass).  Returns with the work enqueued: `stream` is ordered after the share. */
size_t shelfi_combine_share_cts(const shelfi_ctx* ctx, size_t K);
int shelfi_dev_combine_arena(shelfi_ctx* ctx, const uint64_t* arena_dev, const float* w, size_t C, size_t K,
                             size_t pieces, uint64_t* send_dev, uint64_t* share_dev, int fold, void* stream);
/* The same step with the packed share exchange (no reference counterpart): each
 * piece's partial is written packed (the arena's slice format with C = 1, sum_t U_t bits per
 * coefficient) into send_dev, exchanged by one grouped ncclSend/ncclRecv all-to-all into
 * recv_dev, and summed on the comm stream with unit weights (the mod-q fold included) into
 * share_dev.  (W - 1) / W of the packed partial crosses xGMI per rank instead of the uint64 one.
 * send_dev and recv_dev hold shelfi_arena_words(ctx, 1, W * Ks) uint64 words each. */
int shelfi_dev_combine_arena_packed(shelfi_ctx* ctx, const uint64_t* arena_dev, const float* w, size_t C,
                                    size_t K, size_t pieces, uint64_t* send_dev, uint64_t* recv_dev,
                                    uint64_t* share_dev, void* stream);

/* encode + encrypt n doubles (device) into K = ceil(n/batch) ciphertexts. */
int shelfi_dev_encrypt(shelfi_ctx* ctx, const double* x_dev, size_t n, uint64_t* ct_dev,
                       void* stream);
/* decrypt + decode K ciphertexts of scaling factor `scale` into n doubles (device). */
int shelfi_dev_decrypt(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, double scale,
                       size_t n, double* out_dev, void* stream);
/* negacyclic NTT of P polys [P][N] whose tower is (p % L) (PALISADE order).  Inputs are canonical
 * residues below their tower's modulus, outputs are canonical, and P may be any count (not only a
 * multiple of L; 0 is a no-op). */
int shelfi_dev_ntt(shelfi_ctx* ctx, uint64_t* polys_dev, size_t P, int inverse, void* stream);

/* ---- EvalMult (ct x ct), relinearization, ModReduce ---------- *
 * The general-circuit part of the PALISADE 1.11 CKKS scheme behind the reference's
 * contexts (ckks.cpp:28 genCryptoContextCKKS: ks = HYBRID, rs = EXACTRESCALE, dnum from
 * multDepth; the reference's own evaluation key is palisade_pybind/SHELFI_FHE/resources/
 * cryptoparams/key-eval-mult.txt).  Not on the aggregation path (ckks.cpp:26 multDepth = 1).
 * A ciphertext of `towers` RNS towers holds q_0 .. q_{towers-1} (towers = L - level). */
/* Host-only: PALISADE's HYBRID key-switching parameters for a chain: dnum digits of alpha
 * towers and num_special special primes (special/special_roots hold 16). */
int shelfi_special_primes(uint32_t ring_dim, uint32_t num_towers, const uint64_t* moduli, uint32_t* dnum,
                          uint32_t* alpha, uint32_t* num_special, uint64_t* special, uint64_t* special_roots);
/* The context's key-switching parameters; *has_key = 1 once an evaluation key is installed. */
int shelfi_eval_key_info(const shelfi_ctx* ctx, uint32_t* dnum, uint32_t* alpha, uint32_t* num_special,
                         uint64_t* special, int* has_key);
/* cc->EvalMultKeyGen(sk) on the device: the relinearization key s^2 -> s, layout
 * [2][dnum][L + num_special][N] (b-vector, a-vector; EVALUATION), seeded like keygen. */
int shelfi_eval_mult_keygen(shelfi_ctx* ctx);
size_t shelfi_eval_key_words(const shelfi_ctx* ctx); /* 2 * dnum * (L + num_special) * N */
int shelfi_get_eval_key(const shelfi_ctx* ctx, uint64_t* evk);
int shelfi_set_eval_key(shelfi_ctx* ctx, const uint64_t* evk);
/* PALISADE key-eval-mult.txt (cereal archive of the evaluation-key map, as the reference's
 * palisade_pybind/SHELFI_FHE/resources/cryptoparams/key-eval-mult.txt).  save: this context's
 * key (PALISADE keys required: the file embeds their context and key tag); load: a file made
 * for this key pair and these parameters (shelfi_load also picks up a matching
 * key-eval-mult.txt beside the key files). */
int shelfi_save_eval_key(const shelfi_ctx* ctx, const char* path);
int shelfi_load_eval_key(shelfi_ctx* ctx, const char* path);
typedef struct {
  uint32_t ring_dim, num_towers, ctx_towers, dnum; /* num_towers = Q's ctx_towers + special */
  uint64_t moduli[16], roots[16];
  char keytag[257];
} shelfi_palisade_evk_info;
/* Host-only: parse a key-eval-mult.txt; polys [2][dnum][num_towers][ring_dim] when non-NULL. */
int shelfi_palisade_evalkey_parse(const uint8_t* file, size_t len, shelfi_palisade_evk_info* info,
                                  uint64_t* polys);
/* Host-only: the same file re-serialized around other residues (the format's pin). */
int shelfi_palisade_evalkey_rewrite(const uint8_t* file, size_t len, const uint64_t* polys, uint8_t** out,
                                    size_t* out_len);
/* cc->EvalMult(ct_a, ct_b): tensor product + HYBRID relinearization, a, b, out
 * [K][2][towers][N] in HBM (out may be a or b).  Result depth 2, scale = scale_a scale_b. */
int shelfi_dev_mult(shelfi_ctx* ctx, const uint64_t* a_dev, const uint64_t* b_dev, size_t K, uint32_t towers,
                    uint64_t* out_dev, void* stream);
/* cc->EvalInnerProduct's body (EvalMultNoRelin + EvalAddMany + Relinearize) as one call: per tower, in
 * EVALUATION form, c0 = sum_k a_k0 b_k0, c1 = sum_k (a_k0 b_k1 + a_k1 b_k0), c2 = sum_k a_k1 b_k1 mod q_t,
 * and out = (c0, c1) + KeySwitch(c2) under the installed evaluation key -- shelfi_dev_mult's key switch, run
 * once for the whole batch.  a_dev, b_dev [K][2][towers][N], out_dev [1][2][towers][N] in HBM; a_dev == b_dev
 * (the squared norm) reads each ciphertext once and gives the bits the general path gives on a copy.  Result
 * depth 2, scale = scale_a scale_b.  No evaluation key: SHELFI_ERR_STATE.  towers outside 1..L, a NULL buffer,
 * K = 0 (an empty sum has no operand to take a level from), out_dev overlapping either input, and a chain with
 * num_towers + special primes > 16: SHELFI_ERR_ARG.  The K ciphertexts are summed in S = min(16, ceil(K /
 * SHELFI_DOT_SLICE_CTS)) slices (no output bit depends on S).  Uses the context's scratch (the key switch of
 * one ciphertext plus 3 S towers N words) and synchronises `stream` before returning. */
int shelfi_dev_dot(shelfi_ctx* ctx, const uint64_t* a_dev, const uint64_t* b_dev, size_t K, uint32_t towers,
                   uint64_t* out_dev, void* stream);
/* slices S of the last successful shelfi_dev_dot on this context (a refused call leaves it unchanged; for
 * tests of the split) */
uint64_t shelfi_dot_slice_count(const shelfi_ctx* ctx);
/* The Gram matrix of C batches of K ciphertexts, all at one level: out_dev [P][2][towers][N], P = C (C + 1) / 2,
 * holds for every i <= j, at p(i, j) = i C - i (i - 1) / 2 + (j - i) (the upper triangle, row-major), exactly
 * the ciphertext shelfi_dev_dot gives on (batch i, batch j), bit for bit: the pairwise inner products robust
 * aggregation rules need (Krum's distances G_ii + G_jj - 2 G_ij, cosine screening), at one pass over the
 * inputs per tile of 2 x 2 learners and one batched key switch instead of P single ones.  batches_dev: a HOST
 * array of C device pointers [K][2][towers][N] (the same batch may appear twice); the result is a batch of P
 * ordinary ciphertexts of depth 2 and scale = scale^2 for shelfi_dev_rescale, _eval_sum, _add, _sub and the
 * decrypt calls.  No evaluation key: SHELFI_ERR_STATE.  C outside 1..32, K = 0, towers outside 1..L, a NULL
 * pointer, out_dev overlapping any input, and a chain with num_towers + special primes > 16: SHELFI_ERR_ARG.
 * The tiles are cut into launch chains under SHELFI_EVAL_CHUNK_MIB (shelfi_eval_chunk_count reports them);
 * the K ciphertexts are summed in S = min(16, ceil(K / SHELFI_GRAM_SLICE_CTS), ceil(1024 / G)) slices, G =
 * ceil(C / 2) (ceil(C / 2) + 1) / 2 tiles x towers x max(1, N / 512) workgroups a slice: a call is sliced only
 * while its tiles alone leave the machine idle.  No output bit depends on the chains or on S.  Uses the
 * context's scratch and synchronises `stream` before returning. */
int shelfi_dev_gram(shelfi_ctx* ctx, const uint64_t* const* batches_dev, size_t C, size_t K, uint32_t towers,
                    uint64_t* out_dev, void* stream);
/* C (C + 1) / 2: the ciphertexts shelfi_dev_gram writes for C batches */
size_t shelfi_gram_pairs(size_t C);
/* slices S of the last successful shelfi_dev_gram on this context (a refused call leaves it unchanged; for
 * tests of the split) */
uint64_t shelfi_gram_slice_count(const shelfi_ctx* ctx);
/* cc->EvalLinearWSum with ENCRYPTED weights: sum_c w_c u_c over C learners' updates with weights the server
 * cannot read (private dataset-size weights, encrypted selection or clipping factors, encrypted per-parameter
 * masks), at one key switch per OUTPUT ciphertext instead of one per product.  Learner c has an update batch
 * [K][2][u_towers][N] and a weight batch [Kw][2][towers][N], Kw = 1 (one weight ciphertext for its whole update)
 * or Kw = K (one per update ciphertext).  For every k, per tower t < towers, in EVALUATION form, with w = w_{c,0}
 * (Kw = 1) or w_{c,k} (Kw = K): c0 = sum_c w0 u_{c,k,0}, c1 = sum_c (w0 u_{c,k,1} + w1 u_{c,k,0}), c2 = sum_c w1
 * u_{c,k,1} mod q_t, and out[k] = (c0, c1) + KeySwitch(c2) under the installed evaluation key.  out_dev
 * [K][2][towers][N]: ordinary ciphertexts of depth 2 and scale = scale_w scale_u for shelfi_dev_rescale, _add and
 * the decrypt calls.  out[k] is, bit for bit, shelfi_dev_dot of the C stacked weights against the C stacked k-th
 * update ciphertexts, and at C = 1 shelfi_dev_mult of the weight with the update.  u_towers >= towers is part of the
 * contract: weights that come out of a computation sit at a lower level than fresh updates, and the first `towers`
 * towers of each update polynomial are read in place (polynomial stride u_towers N) -- towers [towers, u_towers) are
 * never read, and the result is bit-equal to the call on contiguous prefix copies.  batches_dev, weights_dev: HOST
 * arrays of C device pointers (the same batch may appear twice).  No evaluation key: SHELFI_ERR_STATE.  C outside
 * 1..32 (larger cohorts go in groups through shelfi_dev_add), K = 0, Kw not 1 or K, towers outside 1..u_towers,
 * u_towers > L, a NULL pointer (an array, an entry, out_dev), out_dev overlapping any update batch (over its stored
 * u_towers extent) or any weight batch, and a chain with num_towers + special primes > 16: SHELFI_ERR_ARG; a refused
 * call writes nothing.  The K outputs are cut into launch chains under SHELFI_EVAL_CHUNK_MIB, as shelfi_dev_mult's
 * (shelfi_eval_chunk_count reports them; no output bit depends on them).  Uses the context's scratch (the key switch
 * of a chain's ciphertexts) and synchronises `stream` before returning. */
int shelfi_dev_wsum_ct(shelfi_ctx* ctx, const uint64_t* const* batches_dev, size_t C, size_t K, uint32_t u_towers,
                       const uint64_t* const* weights_dev, size_t Kw, uint32_t towers, uint64_t* out_dev,
                       void* stream);
/* ---- cc->EvalPoly: Paterson-Stockmeyer with four baby steps and one key switch per output ----
 * p(x) = sum_{g < G} x^{4g} q_g(x), deg q_g <= 3, G = ceil((d + 1) / 4) <= 8.  The powers P_1, P_2, P_3 (babies) and
 * P_4, P_8, .. P_{4(G-1)} (giants) come from shelfi_dev_wsum_ct at C = 1 and shelfi_dev_rescale, in the order of
 * the plan; shelfi_dev_poly_combine sums every giant-step product as one tensor and relinearizes it once. */
#define SHELFI_POLY_MAX_DEGREE 31
#define SHELFI_POLY_MAX_GIANTS 8
#define SHELFI_POLY_MAX_POWERS 10 /* P_1, P_2, P_3 and seven giants */
typedef struct shelfi_poly_schedule {
  uint32_t degree, giants /* G */, babies /* min(d, 3) */, rescales /* r of the result: 1 when G = 1, else 2 */;
  uint32_t num_powers;                            /* entries of power_*, every factor before its product */
  uint32_t power_n[SHELFI_POLY_MAX_POWERS];       /* P_n = P_a P_b (n = 1: the input, a = b = 0) */
  uint32_t power_a[SHELFI_POLY_MAX_POWERS], power_b[SHELFI_POLY_MAX_POWERS];
  uint32_t power_towers[SHELFI_POLY_MAX_POWERS];  /* towers P_n is stored with */
  double power_scale[SHELFI_POLY_MAX_POWERS];     /* its exact scale */
  uint32_t combine_towers;                        /* t_c: the least towers over the powers */
  uint32_t result_towers;                         /* t_c - r */
  double combine_scale;                           /* S_c */
  double result_scale;                            /* S_c / q_{t_c - 1} (/ q_{t_c - 2}) */
  double const_scale[SHELFI_POLY_MAX_GIANTS][4];  /* c of term (g, j); 0 where 4 g + j > d */
  uint64_t table[SHELFI_POLY_MAX_GIANTS][4][16];  /* W_{g,j} mod q_t, canonical, t < t_c; 0 elsewhere */
} shelfi_poly_schedule;
/* The plan (host only: no context, no device; the chain is given as for shelfi_special_primes).  moduli[0 ..
 * num_towers) and scale_bits p are the context's (shelfi_ctx_info); coeffs[0 .. degree] the monomial coefficients
 * a_0 .. a_d, 1 <= d <= 31; `towers` and `scale` the input ciphertext's l and s_1; combine_scale S_c, or 0 for the
 * default 2^{2p} (G = 1) / 2^{3p} (G > 1).
 * Schedule: P_2 = P_1 P_1, P_3 = P_2 P_1, P_4 = P_2 P_2, P_{4g} = P_{4h} P_{4(g-h)} with h the largest power of two
 * below g.  A product is one mult at the lower operand's towers t and one rescale: towers t - 1, scale
 * (s_a * s_b) / (double)q_{t-1} in IEEE double in that order; the depth of P_n is ceil(log2 n).
 * Constants: term (g, j) carries a_{4g+j} at the double c = S_c, S_c / s_j, S_c / s_{4g}, (S_c / s_{4g}) / s_j, and
 * W = sign(a) floor(|a| c + 1/2) for the EXACT product of the two doubles; table holds W mod q_t for t < t_c.  Every
 * term of the combine then sits at S_c exactly, whatever the powers' rescales did to their scales.
 * The result of shelfi_dev_poly_combine takes r rescales: towers t_c - r, scale S_c divided by q_{t_c-1} (then
 * q_{t_c-2}) in double.  It costs ceil(log2(highest power)) + r levels: 3 at d = 3, 4 at d = 7, 6 at d = 15.
 * d outside 1..31, a non-finite coefficient, a non-finite or non-positive scale, towers outside 1..num_towers, too
 * few levels (a power below one tower, or t_c - r < 1) and any |W| >= Q_{t_c} / 2: SHELFI_ERR_ARG, *out untouched. */
int shelfi_poly_plan(uint32_t num_towers, const uint64_t* moduli, uint32_t scale_bits, const double* coeffs,
                     uint32_t degree, uint32_t towers, double scale, double combine_scale, shelfi_poly_schedule* out);
/* The combine.  babies_dev[j - 1] = P_j, j = 1..nb (nb = 1..3); giants_dev[g - 1] = P_{4g}, g = 1..ng (ng = 0..7);
 * each a batch [K][2][its towers][N] with its towers (baby_towers / giant_towers) >= `towers`, read in place at its
 * own polynomial stride -- towers at and above `towers` are never touched.  table: HOST words [ng + 1][4][towers],
 * canonical residues of W_{g,j} (entries with j > nb are not read).  Per ciphertext k, tower t < towers and
 * evaluation point, mod q_t, with B_j = P_j and Gamma_g = P_{4g}:
 *   q_{g,0} = W_{g,0} + sum_j W_{g,j} B_{j,0},  q_{g,1} = sum_j W_{g,j} B_{j,1}
 *   d0 = q_{0,0} + sum_{g>=1} Gamma_{g,0} q_{g,0}
 *   d1 = q_{0,1} + sum_{g>=1} (Gamma_{g,0} q_{g,1} + Gamma_{g,1} q_{g,0}),  d2 = sum_{g>=1} Gamma_{g,1} q_{g,1}
 *   out[k] = (d0, d1) + KeySwitch(d2) under the installed evaluation key
 * out_dev [K][2][towers][N]: ciphertexts of depth 2 at the plan's S_c for shelfi_dev_rescale.
 * ng = 0: no tensor and no key switch -- the call needs no evaluation key, takes no scratch and returns with the work
 * enqueued on `stream`.  Otherwise as shelfi_dev_wsum_ct: no evaluation key is SHELFI_ERR_STATE, the K outputs are
 * cut into launch chains under SHELFI_EVAL_CHUNK_MIB (shelfi_eval_chunk_count reports them; no output bit depends
 * on them), the context's scratch is used and `stream` synchronised before returning.
 * nb outside 1..3, ng outside 0..7, towers outside 1..L, an operand stored with fewer than `towers` or more than L
 * towers, K = 0, a NULL pointer (an array, a used entry, table, out_dev), out_dev overlapping any operand over its
 * stored extent, a table entry >= its modulus, and (ng > 0) a chain with num_towers + special primes > 16:
 * SHELFI_ERR_ARG; a refused call writes nothing. */
int shelfi_dev_poly_combine(shelfi_ctx* ctx, const uint64_t* const* babies_dev, const uint32_t* baby_towers,
                            uint32_t nb, const uint64_t* const* giants_dev, const uint32_t* giant_towers, uint32_t ng,
                            const uint64_t* table, size_t K, uint32_t towers, uint64_t* out_dev, void* stream);
/* cc->EvalInnerProduct(ct, pt) (EvalMult(ct, pt) + EvalAddMany) for every pair of C ciphertext batches and R
 * plaintext batches, as one call: out_dev [C R][2][towers][N], entry c R + r, holds per tower, coefficient and
 * component i the canonical sum_k u_{c,k,i} p_{r,k} mod q_t -- the projection of learner c's update on the known
 * vector r (cosine screening against a server update, centred clipping, sketches on public random vectors, and
 * with one-hot plaintexts the packing of many one-number ciphertexts into one).  batches_dev: a HOST array of C
 * device pointers [K][2][towers][N], all at one level (the same batch may appear twice); pts_dev [R][K][towers][N]:
 * R plaintext batches in the layout of shelfi_dev_encode, EVALUATION form, canonical.  Two components, no key of any
 * kind; level and depth are the ciphertexts', scale = scale_ct scale_pt; at C = R = K = 1 the result is
 * shelfi_dev_mult_plain's bit for bit.  C or R outside 1..32, K = 0, towers outside 1..L, a NULL pointer (the array,
 * an entry, pts_dev, out_dev) and out_dev overlapping any input: SHELFI_ERR_ARG; a refused call writes nothing.  A
 * workgroup serves a tile of 2 x 2 (learners x plaintexts), so a learner's batch is read ceil(R / 2) times and a
 * plaintext batch ceil(C / 2) times; at R = 1 the learners go four, then two, then one to a tile (C / 4 + at most 2
 * tiles, the plaintext batch read once for each).  The K ciphertexts are summed
 * in S = min(16, ceil(K / SHELFI_DOTP_SLICE_CTS), ceil(1024 / G)) slices, G = tiles x towers x max(1, N / 512)
 * workgroups a slice, lowered until the partial sums (S C R ciphertexts) fit SHELFI_EVAL_CHUNK_MIB; no output bit
 * depends on the tiles or on S.  With S = 1 the call takes no scratch and returns with the work enqueued on
 * `stream`; with S > 1 it uses the context's scratch and synchronises `stream` before returning. */
int shelfi_dev_project(shelfi_ctx* ctx, const uint64_t* const* batches_dev, size_t C, const uint64_t* pts_dev,
                       size_t R, size_t K, uint32_t towers, uint64_t* out_dev, void* stream);
/* slices S of the last successful shelfi_dev_project (cc->EvalInnerProduct(ct, pt)) on this context (a refused call
 * leaves it unchanged; for tests of the split) */
uint64_t shelfi_dotp_slice_count(const shelfi_ctx* ctx);
/* cc->ModReduce / Rescale: [K][2][towers][N] -> [K][2][towers-1][N] (no overlap), dividing by
 * q_{towers-1} with rounding; scale / q_{towers-1}. */
int shelfi_dev_rescale(shelfi_ctx* ctx, const uint64_t* in_dev, size_t K, uint32_t towers, uint64_t* out_dev,
                       void* stream);
/* shelfi_dev_decrypt for ciphertexts of `towers` <= L towers (after ModReduce). */
int shelfi_dev_decrypt_level(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, uint32_t towers, double scale,
                             size_t n, double* out_dev, void* stream);
/* shelfi_dev_decrypt of a multi-GPU combine's unfolded share: every residue is a uint64 sum of
 * `terms` (1..16) canonical residues (shelfi_dev_combine_arena with fold = 0); the mod-q fold
 * happens inside decrypt's first pass. */
int shelfi_dev_decrypt_sum(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, uint32_t terms, double scale,
                           size_t n, double* out_dev, void* stream);

/* ---- slot rotations and EvalSum (the reference's code/mkhe/mkhe.cpp) -------------- *
 * A rotation by index r is the automorphism X -> X^g, g = 5^r mod 2N (r < 0: the inverse),
 * followed by the HYBRID key switch of EvalMult under a rotation key sigma_g(s) -> s of the
 * evaluation key's layout (shelfi_eval_key_words words).  With this library's encoding it sends
 * slot vector x to out[i] = x[(i + r) mod batch] (r > 0 rotates left), for sparse packing too.
 * A context holds up to 64 rotation keys, keyed by g; a key reload or regeneration
 * (shelfi_keygen, shelfi_load, shelfi_set_keys, shelfi_multiparty_keygen) drops them.  A missing
 * key is SHELFI_ERR_STATE.  Whether PALISADE permutes before or after switching, and its own
 * EvalSumKeyGen index list, are not pinned. */
/* Host-only: PALISADE's FindAutomorphismIndex2nComplex: g = 5^index mod 2N, or its inverse for a
 * negative index; index 0 gives 1.  ring_dim a power of two in 2^2..2^17, |index| < ring_dim / 2. */
int shelfi_galois_element(uint32_t ring_dim, int32_t index, uint32_t* g);
/* cc->EvalAtIndexKeyGen(sk, indices) (mkhe.cpp:124) on the device: adds the rotation keys of n
 * indices (|index| < batch) to those held.  Index 0 is skipped; an index whose key is held is
 * generated again (identically under a seed: the stream is the context's seeded ChaCha20 in a
 * domain of its own, nonce (6 << 56) | (g << 24) | (digit << 16) | (1 + tower), tower field 0
 * for the error).  A 65th key: SHELFI_ERR_ARG. */
int shelfi_rotation_keygen(shelfi_ctx* ctx, const int32_t* indices, size_t n);
/* cc->EvalSumKeyGen(sk) (mkhe.cpp:274): the keys shelfi_dev_eval_sum needs up to n = batch,
 * indices 1, 2, 4, ..., batch / 2. */
int shelfi_eval_sum_keygen(shelfi_ctx* ctx);
/* The indices held (as first given for each g): *n = their count, the first min(cap, *n) in out
 * (out may be NULL when cap is 0). */
int shelfi_rotation_key_indices(const shelfi_ctx* ctx, int32_t* out, size_t cap, size_t* n);
/* Export / import of one rotation key, [2][dnum][L + num_special][N] like the evaluation key (a
 * party of mkhe.cpp:284-317's protocols imports the joint key this way).  A residue >= its
 * modulus: SHELFI_ERR_FORMAT. */
int shelfi_get_rotation_key(const shelfi_ctx* ctx, int32_t index, uint64_t* key);
int shelfi_set_rotation_key(shelfi_ctx* ctx, int32_t index, const uint64_t* key);
/* cc->EvalAtIndex(ct, index): ct_dev, out_dev [K][2][towers][N] in HBM, not overlapping (index 0
 * is a copy; out may then be ct).  Scale and depth are the input's. */
int shelfi_dev_rotate(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, uint32_t towers, int32_t index,
                      uint64_t* out_dev, void* stream);
/* R rotations of the same ciphertexts from ONE digit decomposition (hoisting: PALISADE's
 * EvalFastRotationPrecompute / EvalFastRotation).  With D_j digit j of c1 over Q_l u P in
 * EVALUATION form -- the decomposition shelfi_dev_rotate makes of sigma_g(c1), here made of c1 itself, once --
 * and g_r the Galois element of indices[r]:
 *   out[r] = (sigma_{g_r}(c0), 0) + ModDown(sum_j sigma_{g_r}(D_j) (.) key_{r,j})
 * under the same rotation keys shelfi_dev_rotate uses.  out_dev [R][K][2][towers][N]: every out[r] an ordinary
 * batch at the input's scale and depth.  out[r] decrypts to the slots shelfi_dev_rotate(.., indices[r], ..)
 * gives, within noise, but is NOT bit-equal to it: the approximate basis conversion does not commute with
 * sigma_g.  Indices may repeat; index 0 is a copy of the input.  R = 1..64; R = 0 or K = 0 enqueues nothing.
 * Every key is looked up before anything is enqueued: a missing one is SHELFI_ERR_STATE ("no rotation key for
 * index r") with out_dev untouched.  A NULL pointer, towers outside 1..L, |index| >= batch, R > 64, out_dev
 * overlapping ct_dev, and a chain with num_towers + special primes > 16 (before any key lookup):
 * SHELFI_ERR_ARG.  The K ciphertexts are cut into launch chains under SHELFI_EVAL_CHUNK_MIB, and a list whose
 * accumulators (one set per rotation in flight) would not fit beside one ciphertext's decomposition is cut into
 * rotation groups as well; shelfi_eval_chunk_count reports chains x groups, and no output bit depends on either.
 * The floor of both cuts is one ciphertext with one rotation in flight: where that alone needs more than the budget
 * (its decomposition plus one accumulator set), the chain runs at that size, over the budget, exactly as a
 * one-ciphertext chain of shelfi_dev_rotate does -- the budget bounds the batching, never refuses a call. */
int shelfi_dev_rotate_many(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, uint32_t towers, const int32_t* indices,
                           size_t R, uint64_t* out_dev, void* stream);
/* cc->EvalSum(ct, n) (mkhe.cpp:372), n a power of two in 1..batch: log2(n) steps
 * acc <- acc + Rotate(acc, 2^i), i = 0 .. log2(n) - 1; slot i then holds
 * sum_{j < n} x[(i + j) mod batch].  n = 1 is a copy.  ct_dev and out_dev must not overlap. */
int shelfi_dev_eval_sum(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, uint32_t towers, uint32_t n,
                        uint64_t* out_dev, void* stream);
/* ---- conjugation: the automorphism X -> X^(2N - 1), which conjugates every slot ---- *
 * Its key is a rotation key in all but its Galois element: made in the rotation keys' stream domain (nonce
 * field g = 2N - 1), held among the context's 64 keys (shelfi_rotation_key_indices lists it as index 0) and
 * dropped with them. */
int shelfi_conjugate_keygen(shelfi_ctx* ctx);
/* Export / import, as shelfi_get_rotation_key / shelfi_set_rotation_key (a keyless server is handed it this way). */
int shelfi_get_conjugation_key(const shelfi_ctx* ctx, uint64_t* key);
int shelfi_set_conjugation_key(shelfi_ctx* ctx, const uint64_t* key);
/* out = (sigma_g(c0) + u0, u1), (u0, u1) = KeySwitch(sigma_g(c1)), g = 2N - 1: ct_dev, out_dev [K][2][towers][N] in
 * HBM, not overlapping; chunked like shelfi_dev_rotate.  No key: SHELFI_ERR_STATE, "no conjugation key". */
int shelfi_dev_conjugate(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, uint32_t towers, uint64_t* out_dev,
                         void* stream);
/* The number of launch chains (chunks of the batch, each within the SHELFI_EVAL_CHUNK_MIB scratch budget,
 * 2048 by default) the last successful shelfi_dev_mult, shelfi_dev_gram, shelfi_dev_wsum_ct, shelfi_dev_rescale,
 * shelfi_dev_rotate, shelfi_dev_rotate_many, shelfi_dev_conjugate or shelfi_dev_eval_sum on this context took.  0 after a call that enqueued no chain (K = 0, index 0,
 * n = 1); a refused call leaves it unchanged.  For tests of the chunking. */
uint64_t shelfi_eval_chunk_count(const shelfi_ctx* ctx);
/* cc->EvalAdd(ct_a, ct_b) (mkhe.cpp:168, :368): out = a + b mod q_t over [K][2][towers][N]; out may be a
 * or b.  Needs no keys and no scratch: it returns with the work enqueued on `stream`. */
int shelfi_dev_add(shelfi_ctx* ctx, const uint64_t* a_dev, const uint64_t* b_dev, size_t K, uint32_t towers,
                   uint64_t* out_dev, void* stream);

/* ---- plaintext operands, EvalSub, EvalNegate (PALISADE's SHE calls) ---------- *
 * A plaintext batch is uint64 [Kp][towers][N] in HBM: EVALUATION form, canonical residues < q_t, tower t
 * over q_t of the context's chain, towers in 1..L as for shelfi_dev_decrypt_level.  The API carries no
 * metadata: the caller tracks scales.  None of the six calls needs a key.  towers of 0 or above L, and a
 * NULL buffer with work to do, are SHELFI_ERR_ARG. */
/* cc->MakeCKKSPackedPlaintext (ckks.cpp:80, mkhe.cpp:145) without the Encrypt: n doubles become
 * K = ceil(n / batch) plaintexts, zero-padded like shelfi_dev_encrypt, by the encode inside encrypt
 * exactly: FFTSpecialInv, m_j = round_half_away(fl(fl(v / S) * scale)), reduced into the first `towers`
 * towers, forward NTT.  `scale` is any finite positive double (else SHELFI_ERR_ARG): pass the context's
 * delta for an operand of a fresh ciphertext's scale (add / sub), and (double)q_{towers-1} for a factor
 * whose product is to be rescaled (shelfi_dev_rescale) back to the ciphertext's own scale.
 * |m_j| <= 2^61 is the whole supported range: a larger finite coefficient is SHELFI_ERR_RANGE (PALISADE's
 * approxFactor scale-down, encrypt's large-value path, is not restated for plaintexts), a non-finite one
 * is refused as encrypt refuses it; pt_dev is then unspecified.  Uses the context's scratch in chunks of
 * SHELFI_DEV_CHUNK_MIB (16 * batch + 64 bytes per plaintext) and synchronises `stream` before returning. */
int shelfi_dev_encode(shelfi_ctx* ctx, const double* x_dev, size_t n, uint32_t towers, double scale,
                      uint64_t* pt_dev, void* stream);
/* ---- seeded ciphertexts on the device ---- */
/* Beside cc->Encrypt (ckks.cpp:81): the symmetric encrypt of n doubles into K = ceil(n / batch) seeded
 * ciphertexts -- c0_dev [K][L][N] = NTT(m + e) - a . NTT(s), EVALUATION, canonical, and the call's public
 * seed (32 bytes) from which shelfi_dev_expand_seeded draws c1 = a for ciphertext indices 0 .. K - 1.  e is
 * the e0 of shelfi_dev_encrypt at the same seed and index.  Needs the whole secret key (SHELFI_ERR_STATE
 * without keys or on a threshold share); a coefficient above 2^61 or a non-finite value is
 * SHELFI_ERR_RANGE.  Synchronises `stream` before returning. */
int shelfi_dev_encrypt_seeded(shelfi_ctx* ctx, const double* x_dev, size_t n, uint64_t* c0_dev, uint8_t seed_out[32],
                              void* stream);
/* Polynomial 1 of the batch ct_dev [K][2][towers][N] <- the stream of `seed` for ciphertext indices
 * k0 .. k0 + K - 1 and towers [0, towers): word j of tower t is the 128-bit draw (keygen's) of the
 * ChaCha20 block with key = seed, counter j >> 2, nonce (9 << 56) | (k << 8) | t, mod q_t.  Polynomial 0
 * is left as it is (the caller's c0).  Indices reach 2^48 - 1.  Needs no key; enqueued on `stream`. */
int shelfi_dev_expand_seeded(shelfi_ctx* ctx, uint64_t* ct_dev, size_t K, uint32_t towers, const uint8_t seed[32],
                             uint64_t k0, void* stream);
/* Beside the Deserial of ckks.cpp:281: ciphertext bytes in any wire format (host) -> the batch
 * [K][2][L][N] at out_dev, K the blob's count (shelfi_blob_info); a seeded blob's c1 is expanded.  The
 * header is checked against the context and every landed residue against its modulus
 * (SHELFI_ERR_FORMAT).  Synchronises `stream` before returning. */
int shelfi_dev_blob_unpack(shelfi_ctx* ctx, const uint8_t* blob, size_t len, size_t K, uint64_t* out_dev,
                           void* stream);
/* cc->EvalMult(ct, pt): both components times the plaintext; ct_dev, out_dev [K][2][towers][N], pt_dev
 * [Kp][towers][N] with Kp = K, or Kp = 1 (one plaintext for every ciphertext); any other Kp is
 * SHELFI_ERR_ARG.  Scale: scale_ct * scale_pt.  This and the four calls below need no scratch and
 * return with the work enqueued on `stream`; K = 0 is a no-op; every output residue is canonical; out
 * may be the ciphertext input exactly (either one for shelfi_dev_sub), and must overlap no input
 * otherwise. */
int shelfi_dev_mult_plain(shelfi_ctx* ctx, const uint64_t* ct_dev, const uint64_t* pt_dev, size_t K, size_t Kp,
                          uint32_t towers, uint64_t* out_dev, void* stream);
/* cc->EvalAdd(ct, pt) / cc->EvalSub(ct, pt): c0 +- pt, c1 copied (nothing to copy when out == ct); the
 * plaintext's scale must be the ciphertext's.  Kp as above. */
int shelfi_dev_add_plain(shelfi_ctx* ctx, const uint64_t* ct_dev, const uint64_t* pt_dev, size_t K, size_t Kp,
                         uint32_t towers, uint64_t* out_dev, void* stream);
int shelfi_dev_sub_plain(shelfi_ctx* ctx, const uint64_t* ct_dev, const uint64_t* pt_dev, size_t K, size_t Kp,
                         uint32_t towers, uint64_t* out_dev, void* stream);
/* cc->EvalSub(ct_a, ct_b): out = a - b mod q_t over [K][2][towers][N] (same level and scale). */
int shelfi_dev_sub(shelfi_ctx* ctx, const uint64_t* a_dev, const uint64_t* b_dev, size_t K, uint32_t towers,
                   uint64_t* out_dev, void* stream);
/* cc->EvalNegate(ct): out = -ct mod q_t. */
int shelfi_dev_negate(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, uint32_t towers, uint64_t* out_dev,
                      void* stream);

/* ---- threshold CKKS (the reference's code/mkhe/mkhe.cpp RunCKKS, lines 188-465) ---- *
 * P parties hold additive shares s_i of one secret key; a ciphertext under the joint public key
 * decrypts only when every party contributes a partial decryption.  Encrypt and
 * computeWeightedAverage are unchanged: they work under any public key. */
/* cc->MultipartyKeyGen(prev.publicKey) (mkhe.cpp:268-282): one step of the key chain.  prev_pk is the
 * previous party's public key [2][L][N] (b, a); this party keeps a = prev.a, samples s_i (ternary) and
 * e_i (the context's sigma) from keygen's seeded stream (its a is drawn and dropped) and installs
 * pk = (prev.b + NTT(e_i) - a NTT(s_i), a), sk = NTT(s_i), in memory only.  The lead party calls
 * shelfi_keygen(ctx, ""); after the chain every party installs the last public key beside its own
 * share with shelfi_set_keys(pk_joint, sk_i).  A residue >= q_t: SHELFI_ERR_FORMAT. */
int shelfi_multiparty_keygen(shelfi_ctx* ctx, const uint64_t* prev_pk);
/* Standard deviation of the smudging noise every partial decryption adds (PALISADE's MP_SD role;
 * default 2^20).  0 = parity mode: no noise, deterministic partials.  Negative, non-finite or above
 * 2^40: SHELFI_ERR_ARG. */
int shelfi_set_threshold_noise(shelfi_ctx* ctx, double sigma);
/* cc->MultipartyDecryptLead / MultipartyDecryptMain (mkhe.cpp:395-400) with the context's key share:
 * ct_dev [K][2][towers][N] -> out_dev [K][towers][N] (EVALUATION), lead = 1: c0 + c1 s_i + NTT(e),
 * lead = 0: c1 s_i + NTT(e); e = round(sigma z), one integer polynomial per ciphertext from the
 * context's ChaCha20 stream, nonce (5 << 56) | (g0 + k), g0 a per-context counter that advances by K
 * with every call.  towers in 1..L as for shelfi_dev_decrypt_level; needs keys; synchronises `stream`. */
int shelfi_dev_partial_decrypt(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, uint32_t towers, int lead,
                               uint64_t* out_dev, void* stream);
/* cc->MultipartyDecryptFusion (mkhe.cpp:402): partials_dev is a host array of P (1..16) device
 * pointers, each [K][towers][N]; they are summed mod q_t while decrypt's first pass loads them, and the
 * rest is shelfi_dev_decrypt_level's chain (tower prefix, range flag and exact redo,
 * shelfi_set_decode_exact, decode flooding, shelfi_decode_redo_count, shelfi_decode_log_error).
 * Needs no keys: the fusing party is the server. */
int shelfi_dev_fuse_decrypt(shelfi_ctx* ctx, const uint64_t* const* partials_dev, size_t P, size_t K,
                            uint32_t towers, double scale, size_t n, double* out_dev, void* stream);
/* The same over bytes (mkhe.cpp:395-402).  shelfi_partial_decrypt takes a ciphertext batch in any of the
 * three wire formats and answers with a partial-decryption blob (magic "SHPD": the ciphertext blob's
 * 64-byte header, the joint key's key_id, a lead/main mark, K x L x N uint64 residues; free with
 * shelfi_free).  shelfi_fuse_decrypt takes the scale from the headers and returns SHELFI_ERR_FORMAT
 * unless params_id, key_id, K, depth and scale agree across the partials and exactly one is the lead's. */
int shelfi_partial_decrypt(shelfi_ctx* ctx, const uint8_t* blob, size_t len, int lead, uint8_t** out,
                           size_t* out_len);
int shelfi_fuse_decrypt(shelfi_ctx* ctx, const uint8_t* const* partials, const size_t* lens, size_t P, size_t n,
                        double* out);
/* Host-only: a partial-decryption blob's header (mkhe.cpp:395-400's results as they travel), and the
 * blob built from host residues [K][num_towers][ring_dim] with the given metadata. */
int shelfi_partial_blob_info(const uint8_t* blob, size_t len, uint64_t* num_cts, uint32_t* towers, int* lead,
                             double* scale, uint64_t* key_id);
int shelfi_partial_blob_pack(uint32_t ring_dim, uint32_t num_towers, uint32_t batch, uint64_t num_cts,
                             uint32_t depth, double scale, uint64_t params_id, uint64_t key_id, int lead,
                             const uint64_t* residues, uint8_t** out, size_t* out_len);

/* ---- multiparty evaluation keys for threshold CKKS (mkhe.cpp:271-317) ---- *
 * The parties make the joint EvalMult, rotation and EvalSum keys of s = sum s_i without anybody
 * holding s.  Keys are host arrays of shelfi_eval_key_words words, [2][dnum][L + num_special][N]
 * (b-vector, a-vector), EVALUATION.  These calls install nothing: the joint keys go to
 * shelfi_set_eval_key / shelfi_set_rotation_key.  Common answers: no key pair SHELFI_ERR_STATE; a
 * chain with num_towers + special primes > 16, a word >= its tower's modulus in an imported key,
 * NULL ctx / out: SHELFI_ERR_ARG. */
/* Round 1, one party's share: b_j = NTT(e_j) - a_j s_i + [digit j] P s'_i.  index = 0: the EvalMult
 * share, s' = s_i -- cc->KeySwitchGen(sk, sk) (mkhe.cpp:271) for the lead party, cc->MultiKeySwitchGen
 * (mkhe.cpp:296) for the others.  index != 0 (|index| < batch): the rotation share of that index,
 * s' = sigma_g(s_i) -- one index of cc->MultiEvalSumKeyGen (mkhe.cpp:284; cc->EvalSumKeyGen, :274, for
 * the lead).  prev = NULL: the lead party draws a_j; otherwise a_j is copied from prev's a-vector.
 * Stream: the context's ChaCha20 key, nonce (7 << 56) | (g << 24) | (digit << 16) | (1 + tower) (tower
 * field 0 for e_j; g = 1 for index 0). */
int shelfi_multi_key_switch_gen(shelfi_ctx* ctx, int32_t index, const uint64_t* prev, uint64_t* out);
/* The sum of n (1..16) keys mod q_t.  sum_a = 0: cc->MultiAddEvalKeys (mkhe.cpp:298) /
 * cc->MultiAddEvalSumKeys (mkhe.cpp:288) -- the b-vectors are summed, the a-vectors must be identical
 * (else SHELFI_ERR_ARG) and are kept.  sum_a = 1: cc->MultiAddEvalMultKeys (mkhe.cpp:314) -- both
 * vectors are summed.  Needs no keys. */
int shelfi_multi_add_eval_keys(shelfi_ctx* ctx, const uint64_t* const* keys, size_t n, int sum_a, uint64_t* out);
/* Round 2 of the EvalMult key, cc->MultiMultEvalKey(joint, sk_i) (mkhe.cpp:307, :311): out = (b_j s_i +
 * NTT(E2_j), a_j s_i + NTT(E1_j)); the sum of every party's answer with sum_a = 1 is the EvalMult key
 * of s.  Stream: nonce (8 << 56) | (vector << 24) | (digit << 16). */
int shelfi_multi_mult_eval_key(shelfi_ctx* ctx, const uint64_t* joint, uint64_t* out);

/* ---- test hooks (host-visible tables) ------------------------------------- */
/* CKKS special-FFT twiddles (flat, index lenh + j) as used by the kernels. */
int shelfi_fft_twiddles(uint32_t slots, double* inv_re, double* inv_im, double* fwd_re,
                        double* fwd_im);
/* Gaussian CDT thresholds used by the samplers; returns the entry count. */
int shelfi_gauss_cdt(double sigma, uint64_t* cdt, int max_entries);

#ifdef __cplusplus
}
#endif
#endif /* SHELFI_H_ */
