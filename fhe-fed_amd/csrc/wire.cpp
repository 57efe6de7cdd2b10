// wire.cpp — the three wire formats of a ciphertext batch (uint64 library blob, packed library blob,
// PALISADE archive): the blob header, where a batch's residues lie in host memory (CtLayout), and the
// C ABI's blob and PALISADE file entry points.
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>

#include "api_internal.h"
#include "api_util.h"
#include "palisade_codec.h"
#include "palisade_io.h"

using namespace shelfi;

namespace shelfi {

static BlobHeader parse_blob(const uint8_t* blob, size_t len, const shelfi_ctx* ctx) {
  if (!blob || len < sizeof(BlobHeader)) throw Error{SHELFI_ERR_FORMAT, "ciphertext blob too short"};
  BlobHeader h;
  std::memcpy(&h, blob, sizeof(h));
  // version 1: uint64 residues [K][2][L][N]; version 2: the packed wire payload (the arena's slice
  // format with C = 1, U_t bits per residue: DESIGN.md §3, §5.3); version 3: seeded -- 64 more bytes (the
  // 32-byte public seed, 32 zero bytes), then each ciphertext's c0 as one version-2 group
  if (std::memcmp(h.magic, "SHCT", 4) != 0 || h.version < 1 || h.version > 3 || h.header_bytes != 64)
    throw Error{SHELFI_ERR_FORMAT, "not a SHELFI ciphertext blob (bad magic/version)"};
  if (h.L == 0 || h.L > kMaxTowers || h.logN < 10 || h.logN > 17)
    throw Error{SHELFI_ERR_FORMAT, "corrupt ciphertext blob header"};
  if (ctx) {
    if (h.logN != ctx->p.logN || h.L != ctx->p.L || h.params_id != ctx->params_id)
      throw Error{SHELFI_ERR_FORMAT, "ciphertext was produced under different crypto parameters"};
  }
  const size_t lead = h.version == 3 ? kSeededLeadBytes : sizeof(BlobHeader);
  if (len < lead) throw Error{SHELFI_ERR_FORMAT, "ciphertext blob too short"};
  if (h.version == 3) {
    for (size_t i = sizeof(BlobHeader) + 32; i < lead; ++i)
      if (blob[i]) throw Error{SHELFI_ERR_FORMAT, "seeded ciphertext blob: non-zero padding after the seed"};
    if (h.K >= kSeededMaxCts) throw Error{SHELFI_ERR_FORMAT, "seeded ciphertext blob: 2^48 ciphertexts or more"};
  }
  const uint64_t payload = len - lead;
  if (h.version != 1 && !ctx) {
    // without a context the packed widths are unknown: a ciphertext is 2 (N / 512) rows (seeded: N / 512,
    // its c0 alone) of 64 U bytes for some 32 L <= U <= 60 L
    const uint64_t unit = (h.version == 3 ? 1ull : 2ull) * (1ull << (h.logN - 9)) * 64;
    bool ok = h.K ? payload % h.K == 0 : payload == 0;
    if (ok && h.K) {
      const uint64_t per = payload / h.K;
      ok = per % unit == 0 && per / unit >= 32ull * h.L && per / unit <= 60ull * h.L;
    }
    if (!ok) throw Error{SHELFI_ERR_FORMAT, "ciphertext blob length does not match header"};
    return h;
  }
  // K comes from an untrusted header: bound it by the payload before multiplying, so a
  // forged K whose K * ct_bytes wraps mod 2^64 cannot pass the length check.
  const uint64_t ct_bytes = h.version == 1   ? 2ull * h.L * (8ull << h.logN)
                            : h.version == 2 ? arena_ct_words(ctx->p, 1) * 8
                                             : packed_poly_bytes(ctx->p, ctx->p.L);
  if (h.K > payload / ct_bytes || len != lead + h.K * ct_bytes)
    throw Error{SHELFI_ERR_FORMAT, "ciphertext blob length does not match header"};
  return h;
}

static BlobHeader make_header(const shelfi_ctx* ctx, uint64_t K, uint32_t depth, double scale) {
  const Params& p = ctx->p;
  BlobHeader h;
  std::memset(&h, 0, sizeof(h));
  std::memcpy(h.magic, "SHCT", 4);
  h.version = 1;
  h.header_bytes = 64;
  h.logN = p.logN;
  h.L = p.L;
  h.K = K;
  h.depth = depth;
  h.level = 0;
  h.scale = scale;
  h.params_id = ctx->params_id;
  h.key_id = ctx->key_id;
  h.batch = p.batch;
  h.encoding = 4;
  return h;
}

// A partial decryption's blob ("SHPD", api_internal.h); ctx = nullptr: the header and length alone.
BlobHeader parse_partial(const uint8_t* blob, size_t len, const shelfi_ctx* ctx) {
  if (!blob || len < sizeof(BlobHeader)) throw Error{SHELFI_ERR_FORMAT, "partial decryption blob too short"};
  BlobHeader h;
  std::memcpy(&h, blob, sizeof(h));
  if (std::memcmp(h.magic, "SHPD", 4) != 0 || h.version != 1 || h.header_bytes != 64)
    throw Error{SHELFI_ERR_FORMAT, "not a SHELFI partial decryption blob (bad magic/version)"};
  if (h.L == 0 || h.L > kMaxTowers || h.logN < 10 || h.logN > 17 || h.level > 1)
    throw Error{SHELFI_ERR_FORMAT, "corrupt partial decryption blob header"};
  if (ctx && (h.logN != ctx->p.logN || h.L != ctx->p.L || h.params_id != ctx->params_id))
    throw Error{SHELFI_ERR_FORMAT, "partial decryption was produced under different crypto parameters"};
  // K comes from an untrusted header: bound it by the payload before multiplying
  const uint64_t payload = len - sizeof(BlobHeader), ct_bytes = (uint64_t)h.L * (8ull << h.logN);
  if (h.K > payload / ct_bytes || payload != h.K * ct_bytes)
    throw Error{SHELFI_ERR_FORMAT, "partial decryption blob length does not match header"};
  return h;
}

BlobHeader make_partial_header(const shelfi_ctx* ctx, uint64_t K, uint32_t depth, double scale, bool lead) {
  BlobHeader h = make_header(ctx, K, depth, scale);
  std::memcpy(h.magic, "SHPD", 4);
  h.level = lead ? 1 : 0;
  return h;
}

// Packed wire payload sizes (version-2 blobs): bytes of one (ct, poly) group of the first Lu towers.
uint64_t packed_poly_bytes(const Params& p, uint32_t Lu) {
  const ArenaPack ap = arena_pack(p);
  uint64_t u = 0;
  for (uint32_t t = 0; t < Lu; ++t) u += ap.w[t];
  return (uint64_t)(p.N / kArenaChunk) * 64 * u;
}
// The widths of the first Lu towers (the buffers a prefix upload unpacks)
ArenaPack arena_pack_prefix(const Params& p, uint32_t Lu) {
  Params q = p;
  q.L = Lu;
  return arena_pack(q);
}

// A caller's ciphertext batch, validated against the context (params and key).
CtLayout open_cts(const shelfi_ctx* ctx, const uint8_t* b, size_t len) {
  CtLayout v;
  v.base = const_cast<uint8_t*>(b);
  if (b && palisade_looks_like_archive(b, len)) {
    PalisadeArchive A = palisade_parse_archive(b, len);
    v.pal = true;
    v.K = A.K;
    if (A.K) {
      const Params& p = ctx->p;
      bool same = A.N == p.N && A.L == p.L;
      for (uint32_t t = 0; same && t < p.L; ++t) same = A.q[t] == p.q[t];
      if (!same)
        throw Error{SHELFI_ERR_FORMAT, "PALISADE ciphertexts were produced under different crypto parameters"};
      if (ctx->pal_keytag.empty() || A.keytag != ctx->pal_keytag)
        throw Error{SHELFI_ERR_FORMAT, "PALISADE ciphertexts were encrypted under a different key (keyTag)"};
      if (A.encoding != 4) throw Error{SHELFI_ERR_FORMAT, "PALISADE ciphertexts are not CKKS-packed"};
    }
    v.depth = (uint32_t)A.depth;
    v.level = A.level;
    v.scale = A.scale;
    v.off = std::move(A.tower_off);
    return v;
  }
  BlobHeader h = parse_blob(b, len, ctx);
  v.packed = h.version == 2;
  v.seeded = h.version == 3;
  if (v.seeded) std::memcpy(v.seed, b + sizeof(BlobHeader), 32);  // eight little-endian words
  v.K = h.K;
  v.depth = h.depth;
  v.level = h.level;
  v.scale = h.scale;
  if (v.K && h.key_id != ctx->key_id)
    throw Error{SHELFI_ERR_FORMAT, "ciphertext was encrypted under a different key"};
  return v;
}

// Size of (and, with buf, the header / framing of) an output batch in format fmt; returns its layout.
CtLayout make_output(const shelfi_ctx* ctx, int fmt, uint64_t K, uint32_t depth, uint64_t level, double scale,
                     uint8_t* buf, size_t* total, const uint32_t* seed) {
  const bool pal = fmt == 1;
  CtLayout v;
  if (seed) std::memcpy(v.seed, seed, sizeof(v.seed));
  v.base = buf;
  v.pal = pal;
  v.packed = fmt == 2;
  v.seeded = fmt == 3;
  v.K = K;
  v.depth = depth;
  v.level = level;
  v.scale = scale;
  const Params& p = ctx->p;
  if (pal) {
    if (ctx->pal_ctx_obj.empty())
      throw Error{SHELFI_ERR_STATE, "PALISADE wire format needs keys loaded from PALISADE files"};
    // key_params: what the reference writes (its keys always come from key-public.txt)
    v.off = palisade_layout(ctx->pal_ctx_obj, ctx->pal_keytag, p.N, p.L, p.q, K, depth, level, scale,
                            4, true, true, buf, total);
    return v;
  }
  if (v.seeded && K >= kSeededMaxCts) throw Error{SHELFI_ERR_ARG, "seeded wire format: 2^48 ciphertexts or more"};
  *total = v.seeded ? kSeededLeadBytes + K * packed_poly_bytes(p, p.L)
                    : sizeof(BlobHeader) + K * (v.packed ? 2 * packed_poly_bytes(p, p.L) : 2ull * p.L * p.N * 8);
  if (buf) {
    BlobHeader h = make_header(ctx, K, depth, scale);
    if (v.packed) h.version = 2;
    if (v.seeded) h.version = 3;
    std::memcpy(buf, &h, sizeof(h));
    if (v.seeded) {  // the seed, then the padding that keeps the payload's alignment
      std::memcpy(buf + sizeof(h), v.seed, 32);
      std::memset(buf + sizeof(h) + 32, 0, kSeededLeadBytes - sizeof(h) - 32);
    }
  }
  return v;
}

}  // namespace shelfi

extern "C" {

int shelfi_blob_version(const uint8_t* blob, size_t len, uint32_t* version) {
  if (!version) return SHELFI_ERR_ARG;
  return guarded([&] { *version = parse_blob(blob, len, nullptr).version; });
}

int shelfi_blob_info(const uint8_t* blob, size_t len, uint64_t* num_cts, uint32_t* depth,
                     double* scale, uint64_t* key_id) {
  return guarded([&] {
    BlobHeader h = parse_blob(blob, len, nullptr);
    if (num_cts) *num_cts = h.K;
    if (depth) *depth = h.depth;
    if (scale) *scale = h.scale;
    if (key_id) *key_id = h.key_id;
  });
}

size_t shelfi_blob_header_bytes(void) { return sizeof(BlobHeader); }

int shelfi_partial_blob_info(const uint8_t* blob, size_t len, uint64_t* num_cts, uint32_t* towers, int* lead,
                             double* scale, uint64_t* key_id) {
  return guarded([&] {
    const BlobHeader h = parse_partial(blob, len, nullptr);
    if (num_cts) *num_cts = h.K;
    if (towers) *towers = h.L;
    if (lead) *lead = (int)h.level;
    if (scale) *scale = h.scale;
    if (key_id) *key_id = h.key_id;
  });
}

int shelfi_partial_blob_pack(uint32_t ring_dim, uint32_t num_towers, uint32_t batch, uint64_t num_cts,
                             uint32_t depth, double scale, uint64_t params_id, uint64_t key_id, int lead,
                             const uint64_t* residues, uint8_t** out, size_t* out_len) {
  if (!out || !out_len || (num_cts && !residues)) return SHELFI_ERR_ARG;
  *out = nullptr;
  *out_len = 0;
  return guarded([&] {
    if (ring_dim < 1024 || ring_dim > (1u << 17) || (ring_dim & (ring_dim - 1)) || num_towers < 1 ||
        num_towers > (uint32_t)kMaxTowers)
      throw Error{SHELFI_ERR_ARG, "partial blob: ring dimension or tower count out of range"};
    const uint64_t ct_bytes = (uint64_t)num_towers * ring_dim * 8;
    if (num_cts > (~0ull - sizeof(BlobHeader)) / ct_bytes) throw Error{SHELFI_ERR_ARG, "partial blob: too large"};
    BlobHeader h;
    std::memset(&h, 0, sizeof(h));
    std::memcpy(h.magic, "SHPD", 4);
    h.version = 1;
    h.header_bytes = 64;
    h.logN = (uint32_t)__builtin_ctz(ring_dim);
    h.L = num_towers;
    h.K = num_cts;
    h.depth = depth;
    h.level = lead ? 1 : 0;
    h.scale = scale;
    h.params_id = params_id;
    h.key_id = key_id;
    h.batch = batch;
    h.encoding = 4;
    const size_t payload = (size_t)(num_cts * ct_bytes);
    uint8_t* blob = (uint8_t*)std::malloc(sizeof(h) + payload);
    if (!blob) throw std::bad_alloc();
    std::memcpy(blob, &h, sizeof(h));
    if (payload) std::memcpy(blob + sizeof(h), residues, payload);
    *out = blob;
    *out_len = sizeof(h) + payload;
  });
}

// Host restatement of blob_unpack_kernel (the packed wire payload): row r of the
// [K][2][L][N] batch, lane l, field j -> residue 128 (j >> 1) + 2 l + (j & 1).
int shelfi_blob_unpack(const shelfi_ctx* ctx, const uint8_t* blob, size_t len, uint64_t* out) {
  if (!ctx || !blob || !out) return SHELFI_ERR_ARG;
  return guarded([&] {
    const BlobHeader h = parse_blob(blob, len, ctx);
    const Params& p = ctx->p;
    const uint8_t* pay = blob + sizeof(BlobHeader);
    if (h.version == 1) {
      std::memcpy(out, pay, h.K * 2ull * p.L * p.N * 8);
      return;
    }
    if (h.version == 3)  // c1 is a ChaCha20 stream, which the host does not run
      throw Error{SHELFI_ERR_ARG, "a seeded blob is expanded on the device: use shelfi_dev_blob_unpack (device.from_blob)"};
    const ArenaPack ap = arena_pack(p);
    const uint32_t rpt = p.N / kArenaChunk;
    size_t off = 0;  // dwords
    const uint32_t* w = reinterpret_cast<const uint32_t*>(pay);
    uint64_t* o = out;
    for (uint64_t g = 0; g < h.K * 2; ++g)
      for (uint32_t t = 0; t < p.L; ++t) {
        const uint32_t U = ap.w[t], B = U & ~3u, F = U & 1u, D = B / 4;
        const uint32_t N4 = D / 4, H2 = (D % 4) >= 2 ? 1 : 0, H1 = D & 1;
        const uint32_t O2 = N4 * 256, O1 = O2 + H2 * 128;
        for (uint32_t c = 0; c < rpt; ++c, off += 16 * U, o += kArenaChunk) {
          const uint32_t* sl = w + off;
          for (uint32_t lane = 0; lane < 64; ++lane) {
            uint32_t d[15] = {0};
            for (uint32_t q = 0; q < N4; ++q)
              for (uint32_t i = 0; i < 4; ++i) d[4 * q + i] = sl[q * 256 + 4 * lane + i];
            if (H2) {
              d[4 * N4] = sl[O2 + 2 * lane];
              d[4 * N4 + 1] = sl[O2 + 2 * lane + 1];
            }
            if (H1) d[D - 1] = sl[O1 + lane];
            const uint32_t fl = F ? reinterpret_cast<const uint8_t*>(sl)[64 * B + lane] : 0;
            for (uint32_t j = 0; j < 8; ++j) {
              const uint32_t bo = j * B, i = bo >> 5, sh = bo & 31;
              uint64_t v = (uint64_t)d[i] >> sh;
              if (sh + B > 32) v |= (uint64_t)d[i + 1] << (32 - sh);
              if (sh + B > 64) v |= (uint64_t)d[i + 2] << (64 - sh);
              v &= (1ull << B) - 1;
              if (F) v |= (uint64_t)((fl >> j) & 1u) << B;
              o[128 * (j >> 1) + 2 * lane + (j & 1)] = v;
            }
          }
        }
      }
  });
}

int shelfi_blob_pack(const shelfi_ctx* ctx, const uint64_t* residues, uint64_t K, uint32_t depth,
                     double scale, uint8_t** out, size_t* out_len) {
  if (!ctx || !out || !out_len || (K && !residues)) return SHELFI_ERR_ARG;
  return guarded([&] {
    const Params& p = ctx->p;
    const size_t payload = K * 2ull * p.L * p.N * 8;
    const BlobHeader h = make_header(ctx, K, depth, scale);
    uint8_t* blob = (uint8_t*)std::malloc(sizeof(h) + payload);
    if (!blob) throw std::bad_alloc();
    std::memcpy(blob, &h, sizeof(h));
    if (payload) std::memcpy(blob + sizeof(h), residues, payload);
    *out = blob;
    *out_len = sizeof(h) + payload;
  });
}

// ------------------------------------------------- PALISADE wire format ----
int shelfi_set_wire_format(shelfi_ctx* ctx, int format) {
  if (!ctx || format < 0 || format > 3) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    if (format == 1 && ctx->pal_ctx_obj.empty())
      throw Error{SHELFI_ERR_STATE, "PALISADE wire format needs keys loaded from PALISADE files"};
    ctx->wire = format;
  });
}

int shelfi_get_wire_format(const shelfi_ctx* ctx) {
  if (!ctx) return -1;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return ctx->wire;
}

int shelfi_palisade_parse(const uint8_t* archive, size_t len, shelfi_palisade_info* info,
                          uint64_t* residues) {
  if (!archive || !info) return SHELFI_ERR_ARG;
  return guarded([&] {
    const PalisadeArchive A = palisade_parse_archive(archive, len);
    std::memset(info, 0, sizeof(*info));
    info->ring_dim = A.N;
    info->num_towers = A.L;
    info->num_cts = A.K;
    for (uint32_t t = 0; t < A.L; ++t) info->moduli[t] = A.q[t];
    info->depth = A.depth;
    info->level = A.level;
    info->scale = A.scale;
    info->encoding = A.encoding;
    info->vector_archive = A.vector_archive ? 1 : 0;
    info->ctx_offset = A.ctx_off;
    info->ctx_length = A.ctx_len;
    std::memcpy(info->keytag, A.keytag.data(), std::min<size_t>(A.keytag.size(), 256));
    if (residues)
      for (size_t i = 0; i < A.tower_off.size(); ++i)
        std::memcpy(residues + i * (size_t)A.N, archive + A.tower_off[i], (size_t)A.N * 8);
  });
}

int shelfi_palisade_write(const uint8_t* ctx_obj, size_t ctx_len, const char* keytag,
                          uint32_t ring_dim, uint32_t num_towers, const uint64_t* moduli,
                          uint64_t num_cts, const uint64_t* residues, uint64_t depth, uint64_t level,
                          double scale, int flags, uint8_t** out, size_t* out_len) {
  if (!ctx_obj || !keytag || !moduli || !out || !out_len || (num_cts && !residues) ||
      num_towers < 1 || num_towers > (uint32_t)kMaxTowers)
    return SHELFI_ERR_ARG;
  *out = nullptr;
  *out_len = 0;
  return guarded([&] {
    const std::string obj((const char*)ctx_obj, ctx_len), tag(keytag);
    const bool vec = (flags & SHELFI_PAL_VECTOR) != 0, kp = (flags & SHELFI_PAL_KEY_PARAMS) != 0;
    size_t total = 0;
    palisade_layout(obj, tag, ring_dim, num_towers, moduli, num_cts, depth, level, scale, 4, vec, kp,
                    nullptr, &total);
    uint8_t* buf = (uint8_t*)std::malloc(total);
    if (!buf) throw std::bad_alloc();
    const std::vector<size_t> off = palisade_layout(obj, tag, ring_dim, num_towers, moduli, num_cts,
                                                    depth, level, scale, 4, vec, kp, buf, &total);
    for (size_t i = 0; i < off.size(); ++i)
      std::memcpy(buf + off[i], residues + i * (size_t)ring_dim, (size_t)ring_dim * 8);
    *out = buf;
    *out_len = total;
  });
}

static void take_string(const std::string& s, uint8_t** out, size_t* out_len) {
  uint8_t* buf = (uint8_t*)std::malloc(s.size() ? s.size() : 1);
  if (!buf) throw std::bad_alloc();
  std::memcpy(buf, s.data(), s.size());
  *out = buf;
  *out_len = s.size();
}

int shelfi_palisade_context_file(uint32_t ring_dim, uint32_t num_towers, const uint64_t* moduli,
                                 const uint64_t* roots, uint32_t scale_bits, uint32_t batch,
                                 uint8_t** out, size_t* out_len) {
  if (!moduli || !roots || !out || !out_len || num_towers < 1 || num_towers > (uint32_t)kMaxTowers)
    return SHELFI_ERR_ARG;
  *out = nullptr;
  return guarded([&] {
    PalisadeCtxParams cp;
    cp.N = ring_dim;
    cp.L = num_towers;
    cp.q.assign(moduli, moduli + num_towers);
    cp.psi.assign(roots, roots + num_towers);
    cp.plaintext_modulus = scale_bits;
    cp.batch = batch;
    take_string(palisade_context_file(cp), out, out_len);
  });
}

int shelfi_palisade_key_file(const uint8_t* ctx_obj, size_t ctx_len, const char* keytag,
                             const uint64_t* polys, int is_public, uint8_t** out, size_t* out_len) {
  if (!ctx_obj || !keytag || !polys || !out || !out_len) return SHELFI_ERR_ARG;
  *out = nullptr;
  return guarded([&] {
    uint32_t id0 = 0;
    const PalisadeCtxParams cp =
        palisade_parse_context_object(std::string((const char*)ctx_obj, ctx_len), &id0);
    if (id0 != 3) throw Error{SHELFI_ERR_FORMAT, "context object must be in embedded form (ids from 3)"};
    take_string(palisade_key_file(cp, keytag, polys, is_public != 0), out, out_len);
  });
}

int shelfi_palisade_key_context(const uint8_t* pub, size_t len, uint8_t** ctx_obj, size_t* ctx_len,
                                char* keytag) {
  if (!pub || !ctx_obj || !ctx_len || !keytag) return SHELFI_ERR_ARG;
  *ctx_obj = nullptr;
  return guarded([&] {
    std::string obj, tag;
    palisade_key_context(std::string((const char*)pub, len), obj, tag);
    uint8_t* buf = (uint8_t*)std::malloc(obj.size());
    if (!buf) throw std::bad_alloc();
    std::memcpy(buf, obj.data(), obj.size());
    *ctx_obj = buf;
    *ctx_len = obj.size();
    std::memset(keytag, 0, 257);
    std::memcpy(keytag, tag.data(), std::min<size_t>(tag.size(), 256));
  });
}

int shelfi_palisade_embed_context(const uint8_t* ctxfile, size_t len, uint8_t** out,
                                  size_t* out_len) {
  if (!ctxfile || !out || !out_len) return SHELFI_ERR_ARG;
  *out = nullptr;
  return guarded([&] {
    const std::string obj = palisade_embed_context(std::string((const char*)ctxfile, len));
    uint8_t* buf = (uint8_t*)std::malloc(obj.size());
    if (!buf) throw std::bad_alloc();
    std::memcpy(buf, obj.data(), obj.size());
    *out = buf;
    *out_len = obj.size();
  });
}

}  // extern "C"
