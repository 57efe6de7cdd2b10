// api_internal.h — declarations shared by the C-ABI sources only (context.cpp, wire.cpp, call_state.cpp,
// bytes_api.cpp, dev_api.cpp, dev_arena.cpp, eval_state.cpp, eval_keys.cpp).  The contract with the kernels
// and comm.cpp is shelfi_internal.h; the evaluation state's own declarations are in eval_internal.h.
#pragma once

#include <string.h>

#include <algorithm>
#include <cstdint>
#include <initializer_list>
#include <vector>

#include "api_util.h"
#include "host_stage.h"
#include "shelfi_internal.h"

// Nothing declared here is part of libshelfi.so's dynamic symbol table.
#pragma GCC visibility push(hidden)

namespace shelfi {

// ------------------------------------------------------- chunked calls ----
// Ciphertexts per launch chain of a device call: K split evenly over the fewest chains whose scratch
// (per_ct bytes a ciphertext) fits a budget of budget_mib MiB, so no launch runs a short tail chunk.
inline uint64_t chunk_split(uint64_t K, uint64_t budget_mib, size_t per_ct) {
  const uint64_t cap = std::max<uint64_t>(1, (budget_mib << 20) / std::max<size_t>(per_ct, 1));
  const uint64_t n = (K + cap - 1) / cap;
  return n ? (K + n - 1) / n : 1;
}

// The chunk loop of a device call over K ciphertexts, a chain of kc needing scratch_bytes_of(kc) bytes: the
// context's scratch grown once for the largest chain, then body(k0, kc, scratch) for ciphertexts [k0, k0 + kc)
// of every chain in turn.  Returns the number of chains; they share the scratch, so the caller synchronises
// its stream before the next call.  budget_mib: switches().dev_chunk_mib or switches().eval_chunk_mib.
template <class ScratchBytesOf, class Body>
uint64_t for_chunks(shelfi_ctx* ctx, uint64_t K, uint64_t budget_mib, ScratchBytesOf scratch_bytes_of, Body body) {
  const uint64_t kc_max = chunk_split(K, budget_mib, scratch_bytes_of(1));
  void* scratch = ensure(ctx->scratch, ctx->scratch_bytes, scratch_bytes_of(kc_max));
  uint64_t chains = 0;
  for (uint64_t k0 = 0; k0 < K; k0 += kc_max, ++chains) body(k0, std::min(kc_max, K - k0), scratch);
  return chains;
}

// ------------------------------------------------------ operand checks ----
// do the word ranges [a, a + na) and [b, b + nb) share a word?
inline bool words_overlap(const uint64_t* a, uint64_t na, const uint64_t* b, uint64_t nb) {
  return a < b + nb && b < a + na;
}
// A pointwise call reads each residue before it writes it: its output may be one of its inputs exactly, but
// must not overlap an input at a shift (out and every input `words` words long; a null input is absent).
inline bool out_exact_or_apart(const uint64_t* out, uint64_t words, std::initializer_list<const uint64_t*> ins) {
  for (const uint64_t* in : ins)
    if (in && in != out && words_overlap(in, words, out, words)) return false;
  return true;
}
inline void require_towers(const Params& p, uint32_t towers) {
  if (towers < 1 || towers > p.L) throw Error{SHELFI_ERR_ARG, "tower count out of range for this context"};
}

// ---------------------------------------------------------- context.cpp ----
// the ChaCha20 key of a call that draws randomness: the context's seed, or OS entropy per call
void stream_key(const shelfi_ctx* ctx, uint32_t key[8]);
// encryption stream key + first ciphertext index for this call
void draw_key(shelfi_ctx* ctx, uint64_t count, uint32_t key[8], uint64_t* g0);

// the public seed of a seeded encrypt call: the first eight words of the block (counter 0, nonce
// (9 << 56) | g0) of the call's stream key -- a block no other draw reads
void seeded_seed(const uint32_t key[8], uint64_t g0, uint32_t seed[8]);

// Zeroes a call's stream key when the call leaves its scope, by return or by exception.
struct KeyWiper {
  uint32_t* key;
  explicit KeyWiper(uint32_t k[8]) : key(k) {}
  ~KeyWiper() { explicit_bzero(key, 8 * sizeof(uint32_t)); }
  KeyWiper(const KeyWiper&) = delete;
  KeyWiper& operator=(const KeyWiper&) = delete;
};

// ------------------------------------------------------------- wire.cpp ----
// 64-byte little-endian header followed by K x 2 x L x N uint64 residues in the
// device layout [ct][poly][tower][coeff] (EVALUATION, PALISADE bit-reversed order).
struct BlobHeader {
  char magic[4];           // "SHCT"
  uint16_t version;        // 1
  uint16_t header_bytes;   // 64
  uint32_t logN;
  uint32_t L;
  uint64_t K;              // ciphertexts in the blob
  uint32_t depth;          // PALISADE depth (1 fresh, 2 after EvalMult by constant)
  uint32_t level;          // always 0 (no rescale on this path)
  double scale;            // scaling factor (Delta for fresh, Delta^2 after EvalMult)
  uint64_t params_id;      // hash of (N, L, q)
  uint64_t key_id;         // hash of the public key (PALISADE keyTag analogue)
  uint32_t batch;          // slots per ciphertext
  uint32_t encoding;       // 4 = CKKSPacked (PALISADE PlaintextEncodings)
};
static_assert(sizeof(BlobHeader) == 64, "blob header must be 64 bytes");
// A seeded blob (version 3): the header, the 32-byte public seed, 32 zero bytes, then the payload
constexpr size_t kSeededLeadBytes = 128;
// A partial decryption (threshold scheme) travels under the same 64-byte header with magic "SHPD",
// version 1 and a payload of K x L x N uint64 residues [ct][tower][coeff]: logN, L, K, depth, scale,
// params_id, batch and encoding as in the ciphertexts it was made from, key_id the joint public key's.
// The `level` word (always 0 in a ciphertext blob) carries the role: 1 = lead (c0 + c1 s + e,
// MultipartyDecryptLead), 0 = main (c1 s + e, MultipartyDecryptMain); any other value is refused.
BlobHeader parse_partial(const uint8_t* blob, size_t len, const shelfi_ctx* ctx);
BlobHeader make_partial_header(const shelfi_ctx* ctx, uint64_t K, uint32_t depth, double scale, bool lead);

// Packed wire payload sizes (version-2 blobs): bytes of one (ct, poly) group of the first Lu towers.
uint64_t packed_poly_bytes(const Params& p, uint32_t Lu);
// The widths of the first Lu towers (the buffers a prefix upload unpacks)
ArenaPack arena_pack_prefix(const Params& p, uint32_t Lu);

// Where the residues of a bytes-API ciphertext batch live in host memory: a library
// blob (one contiguous payload) or a PALISADE archive (2*L tower runs per ciphertext,
// palisade_codec.h).  Both map onto the device layout [K][2][L][N].
struct CtLayout {
  uint8_t* base = nullptr;
  bool pal = false;
  bool packed = false;  // a version-2 (packed) library blob
  bool seeded = false;  // a version-3 (seeded) library blob: c0 groups only, c1 expanded from `seed`
  uint32_t seed[8] = {};
  int fmt() const { return pal ? 1 : packed ? 2 : seeded ? 3 : 0; }  // shelfi_set_wire_format's numbering
  uint64_t K = 0;
  uint32_t depth = 0;
  uint64_t level = 0;
  double scale = 0.0;
  std::vector<size_t> off;  // PALISADE tower offsets [K][2][L]
  // ciphertexts [k0, k0 + kn) as host pieces in [K][2][L][N] order; with Lu < L only each
  // polynomial's first Lu towers (the decode's prefix, decode_pass): [kn][2][Lu][N]
  void pieces(uint64_t k0, uint64_t kn, const Params& p, std::vector<HostPiece>& out, uint32_t Lu = 0) const {
    out.clear();
    if (!Lu) Lu = p.L;
    const size_t poly_bytes = (size_t)p.L * p.N * 8, ct_bytes = 2 * poly_bytes;
    if (packed || seeded) {  // (ct, poly) groups of packed rows; a tower prefix is a prefix of each group
      const uint64_t pg = packed_poly_bytes(p, p.L);
      const uint64_t gpc = seeded ? 1 : 2;  // groups per ciphertext: a seeded one carries its c0 alone
      uint8_t* const pay = base + (seeded ? kSeededLeadBytes : sizeof(BlobHeader));
      if (Lu == p.L) {
        out.push_back(HostPiece{pay + k0 * gpc * pg, kn * gpc * pg});
        return;
      }
      const uint64_t pl = packed_poly_bytes(p, Lu);
      for (uint64_t i = gpc * k0; i < gpc * (k0 + kn); ++i) out.push_back(HostPiece{pay + i * pg, (size_t)pl});
      return;
    }
    if (!pal) {
      if (Lu == p.L) {
        out.push_back(HostPiece{base + sizeof(BlobHeader) + k0 * ct_bytes, kn * ct_bytes});
        return;
      }
      for (uint64_t i = 2 * k0; i < 2 * (k0 + kn); ++i)
        out.push_back(HostPiece{base + sizeof(BlobHeader) + i * poly_bytes, (size_t)Lu * p.N * 8});
      return;
    }
    for (uint64_t i = 2 * k0; i < 2 * (k0 + kn); ++i)
      for (uint32_t t = 0; t < Lu; ++t) out.push_back(HostPiece{base + off[i * p.L + t], (size_t)p.N * 8});
  }
};

// A caller's ciphertext batch, validated against the context (params and key).
CtLayout open_cts(const shelfi_ctx* ctx, const uint8_t* b, size_t len);
// Size of (and, with buf, the header / framing of) an output batch in format fmt; returns its layout.
// (seed: the public seed a seeded batch's framing carries)
CtLayout make_output(const shelfi_ctx* ctx, int fmt, uint64_t K, uint32_t depth, uint64_t level, double scale,
                     uint8_t* buf, size_t* total, const uint32_t* seed = nullptr);
// What a batch lands as on the device: a seeded blob's c0 groups (ciphertexts k0 .. of the blob, each
// polynomial's first Lu towers, packed at src) into a [kn][2][Lu][N] batch at dst with c1 expanded beside
// them; ap = arena_pack_prefix(p, Lu).  On the stream s (the compute stream of a pipeline).
void seeded_land(const shelfi_ctx* ctx, const CtLayout& v, const uint8_t* src, uint64_t k0, uint64_t kn, uint32_t Lu,
                 const ArenaPack& ap, uint64_t* dst, hipStream_t s);

// -------------------------------------------------------- bytes_api.cpp ----
// The ctx's pinned staging rings, created on first use
Stager& stager(shelfi_ctx* ctx);

// Drops the staged outputs of a pipeline that threw (declared after its Pipe, so the
// slots are abandoned before the streams are drained).
struct StageRun {
  Stager& s;
  bool done = false;
  explicit StageRun(Stager& st) : s(st) { s.begin(); }
  void finish() {
    s.finish();
    done = true;
  }
  ~StageRun() {
    if (!done) s.abort();
  }
};

// -------------------------------------------------------- dev_arena.cpp ----
// The next slot of the context's ring of small device buffers (shelfi_ctx::wl_*), at least `bytes` large, free to
// be rewritten (the event of its last readers has been waited for).  ctx lock held.  The caller fills
// ctx->wl_dev[slot] by a copy ordered on its stream and records ctx->wl_done[slot] on that stream behind the
// kernels that read it: the slot is handed out again only after that event.
int weight_ring_slot(shelfi_ctx* ctx, size_t bytes);

// ------------------------------------------------------- call_state.cpp ----
// W = (int64)((double)(float)w * Delta + 0.5) mod q_t as two 30-bit limbs, wl[t][2] for the p.L towers
void weight_limbs(float w, const Params& p, uint32_t* wl);
// the same for the n learners of a wavg launch
void fill_weights(WavgArgs& a, const Params& p, const float* w, size_t n);

GenFlag next_gen_flag(shelfi_ctx* ctx);
// after the call's synchronisation: did it raise word w?
bool gen_flag_raised(const shelfi_ctx* ctx, const GenFlag& f, int w);
bool encode_needs_approx(const shelfi_ctx* ctx, const GenFlag& f);

DecodeNoise decode_noise_begin(shelfi_ctx* ctx, uint64_t K, const GenFlag& fl);
// complex slot packing with decode noise enabled: SHELFI_ERR_STATE (decode_noise_begin checks it too)
void require_no_flood_on_complex(const shelfi_ctx* ctx);
// complex slot packing reads / writes a device vector as 16-byte (re, im) words
inline void require_pair_aligned(const shelfi_ctx* ctx, const void* v) {
  if (ctx->p.pack && (reinterpret_cast<uintptr_t>(v) & 15))
    throw Error{SHELFI_ERR_ARG, "complex slot packing needs a 16-byte aligned value vector"};
}
void decode_noise_readback(shelfi_ctx* ctx, const DecodeNoise& dn);
void decode_noise_end(shelfi_ctx* ctx, const DecodeNoise& dn);

// One pass of a decrypt call over ciphertexts of `towers` towers: the parameters and tables of the
// towers it decodes with -- the fast CRT's prefix (decode_towers), or (exact) every tower.
struct DecodePass {
  Params p;
  const DeviceTables& dt;
};
DecodePass decode_pass(shelfi_ctx* ctx, uint32_t towers, bool exact);

// The passes of a decrypt call: run(exact) enqueues one pass over the whole call, wait() returns once
// that pass has completed.  The fast pass first; when it met a coefficient outside the fast CRT's
// range (GenFlag word 2), the call again, exactly (counted in ctx->decode_redo_count; the caller holds
// ctx->mu).  Then the flooding's precision verdict; the flooding key is wiped however the call ends.
// The fast pass of a redone call flooded wrapped values and may have raised the precision word at the
// call's generation, which the exact pass cannot lower: the redo's flooding reports under a generation
// of its own, so the verdict is the exact pass's alone (same key and counters: the same noise stream).
template <class Run, class Wait>
void decrypt_passes(shelfi_ctx* ctx, const GenFlag& fl, DecodeNoise& dn, Run run, Wait wait) {
  KeyWiper wipe(dn.key);
  if (ctx->decode_exact) {
    run(true);
  } else {
    run(false);
    wait();
    if (gen_flag_raised(ctx, fl, 2)) {
      ++ctx->decode_redo_count;
      if (dn.enabled) dn.fail = next_gen_flag(ctx);
      run(true);
    }
  }
  wait();
  decode_noise_end(ctx, dn);
}

// ---------------------------------------------------------- dev_api.cpp ----
// The device decrypt driver and the threshold partial decryption behind the shelfi_dev_* entry points,
// for the bytes API as well (the caller holds ctx->mu, has selected the device and checked the keys;
// both return with `s` synchronised).  fuse: threshold fusion of fuse->P partials, no ct_dev, no keys.
void dev_decrypt_locked(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, uint32_t towers, double scale, size_t n,
                        double* out_dev, hipStream_t s, bool sum_in, const FuseIn* fuse);
void partial_decrypt_locked(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, uint32_t towers, bool lead,
                            uint64_t* out_dev, hipStream_t s);

}  // namespace shelfi

#pragma GCC visibility pop
