// call_state.cpp — what the bytes API (bytes_api.cpp) and the device API (dev_api.cpp) share about one
// call: the learners' weights, the call's generation of the GenFlag words, decode noise flooding and
// the decode's tower prefix.
#include <cmath>
#include <cstring>
#include <mutex>

#include "api_internal.h"
#include "api_util.h"
#include "eval_internal.h"

using namespace shelfi;

namespace shelfi {

// W = (int64)((double)(float)w * Delta + 0.5) (ckks.cpp:287-288, PALISADE EvalMult by a
// constant). The cast is undefined for NaN, +-inf and |w * Delta| >= 2^63, so such weights
// are rejected instead of producing a garbage aggregate.
static int64_t weight_int(float w, double delta) {
  const double v = (double)w * delta + 0.5;
  if (!std::isfinite(v) || v >= 9223372036854775808.0 || v < -9223372036854775808.0)
    throw Error{SHELFI_ERR_RANGE, "scaling factor is not finite or |w * scale| >= 2^63"};
  return (int64_t)v;
}

void check_wavg_weights(const float* w, size_t C, double delta) {
  for (size_t c = 0; c < C; ++c) (void)weight_int(w[c], delta);
}

// W mod q_t per tower, split into 30-bit limbs
void weight_limbs(float w, const Params& p, uint32_t* wl) {
  const int64_t W = weight_int(w, p.delta);  // ckks.cpp:287-288
  for (uint32_t t = 0; t < p.L; ++t) {
    const uint64_t wt = mod_signed(W, p.q[t]);
    wl[2 * t] = (uint32_t)(wt & ((1u << 30) - 1));
    wl[2 * t + 1] = (uint32_t)(wt >> 30);
  }
}
void fill_weights(WavgArgs& a, const Params& p, const float* w, size_t n) {
  for (size_t c = 0; c < n; ++c) weight_limbs(w[c], p, &a.wl[c][0][0]);
}

// RFC 8439's block function as the kernels run it (dev_common.h chacha20_block: a 64-bit counter in words
// 12-13, a 64-bit nonce in words 14-15), for the one block a seeded encrypt call derives its seed from.
static void chacha20_block_host(const uint32_t key[8], uint64_t counter, uint64_t nonce, uint32_t out[16]) {
  const uint32_t s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key[0], key[1], key[2], key[3],
                          key[4], key[5], key[6], key[7], (uint32_t)counter, (uint32_t)(counter >> 32),
                          (uint32_t)nonce, (uint32_t)(nonce >> 32)};
  uint32_t x[16];
  std::memcpy(x, s, sizeof(x));
  const auto rotl = [](uint32_t v, int n) { return (v << n) | (v >> (32 - n)); };
  const auto qr = [&](int a, int b, int c, int d) {
    x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 16);
    x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 12);
    x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 8);
    x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 7);
  };
  for (int i = 0; i < 10; ++i) {
    qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15);
    qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14);
  }
  for (int i = 0; i < 16; ++i) out[i] = x[i] + s[i];
}

void seeded_seed(const uint32_t key[8], uint64_t g0, uint32_t seed[8]) {
  uint32_t blk[16];
  chacha20_block_host(key, 0, (9ull << 56) | g0, blk);
  std::memcpy(seed, blk, 32);
  explicit_bzero(blk, sizeof(blk));
}

void seeded_land(const shelfi_ctx* ctx, const CtLayout& v, const uint8_t* src, uint64_t k0, uint64_t kn, uint32_t Lu,
                 const ArenaPack& ap, uint64_t* dst, hipStream_t s) {
  const Params& p = ctx->p;
  launch_blob_unpack_groups((const uint32_t*)src, kn, Lu, p.logN, ap, dst, 2ull * Lu * p.N, s);
  launch_seeded_expand(v.seed, k0, kn, Lu, p.logN, ctx->dt.tc, dst, s);
}

// A call's generation of the GenFlag words (shelfi_internal.h).  Every caller synchronises before the next
// call starts, so no kernel writes the words while the host clears them at a wrap of the counter.
GenFlag next_gen_flag(shelfi_ctx* ctx) {
  if (++ctx->map_gen == 0) {
    std::memset(ctx->map_flag_host, 0, 64);
    ctx->map_gen = 1;
  }
  return GenFlag{ctx->map_flag_dev, ctx->map_gen};
}
bool gen_flag_raised(const shelfi_ctx* ctx, const GenFlag& f, int w) {
  return __atomic_load_n(ctx->map_flag_host + w, __ATOMIC_ACQUIRE) == f.gen;
}

// The encode range flag of an encrypt call (encrypt.hip enc_range_flag): non-finite values are refused;
// a finite message coefficient above 2^61 in magnitude means the call is redone on the large-value path
// (the callers count that in ctx->encode_redo_count).
bool encode_needs_approx(const shelfi_ctx* ctx, const GenFlag& f) {
  if (gen_flag_raised(ctx, f, 1)) throw Error{SHELFI_ERR_RANGE, "encrypt: non-finite input value"};
  return gen_flag_raised(ctx, f, 0);
}

// Noise-flooding setup for one decrypt of K ciphertexts (enabled by
// shelfi_set_decode_noise); its randomness comes from the ctx stream like encrypt's.
// Complex slot packing has no flooded decode: PALISADE's flooding estimates sigma from the imaginary parts,
// which then carry data.  Refused before anything is enqueued, never decoded without the
// noise the caller asked for.
void require_no_flood_on_complex(const shelfi_ctx* ctx) {
  if (ctx->p.pack && ctx->decode_noise)
    throw Error{SHELFI_ERR_STATE,
                "decode noise flooding cannot run on complex slot packing: call set_decode_noise(False) "
                "(shelfi_set_decode_noise(ctx, 0, 1.0)) before decrypting; threshold smudging is unaffected"};
}

DecodeNoise decode_noise_begin(shelfi_ctx* ctx, uint64_t K, const GenFlag& fl) {
  DecodeNoise dn;
  require_no_flood_on_complex(ctx);
  if (!ctx->decode_noise) return dn;
  dn.fail = fl;
  dn.enabled = 1;
  dn.m_factor = ctx->decode_m_factor;
  dn.p_bits = ctx->p.scale_bits;
  draw_key(ctx, K, dn.key, &dn.g0);
  dn.flags = ctx->dev_flag;
  // flag [2] (logError) is reset by the first chunk's flooding (launch_decrypt: inside
  // decode_stats_kernel, or a fill before the small-ring decode_flood_kernel)
  return dn;
}

// After a flooded decrypt was enqueued: its logError (device flag [2]) is read back only when asked for
// (shelfi_decode_log_error), not after every call; the precision failure is a GenFlag word (round 6).
void decode_noise_readback(shelfi_ctx* ctx, const DecodeNoise& dn) {
  if (dn.enabled) ctx->log_error_pending = true;
}

// After the decrypt's stream work has completed: raise PALISADE's precision failure (Decode throws
// math_error when log2 sigma > p - 5).
void decode_noise_end(shelfi_ctx* ctx, const DecodeNoise& dn) {
  if (dn.enabled && gen_flag_raised(ctx, dn.fail, 3))
    throw Error{SHELFI_ERR_PRECISION,
                "The decryption failed because the approximation error is too high. Check the "
                "parameters."};
}

// Towers the decode's fast path reads: the shortest prefix of q_0 .. q_{towers-1} whose product
// exceeds 2^130.  crt_value decodes X exactly over that prefix Q' while |X| < 2^127: the centred
// residue of X mod Q' is X itself, and |X| / Q' < 2^-3 keeps k's estimate clear of its rounding
// boundary, so the towers past the prefix change no output bit.  A coefficient
// outside that range sets the CRT range flag and the call is redone over every tower through
// crt_exact_kernel (round 6), as PALISADE's BigInteger decode, up to (Q - 1) / 2.  2^15 / L4
// (60 + 3 x 52 bits): 3 of 4 towers.  A chain at or below 2^130 (multDepth = 1: 60 + 52 bits; one or
// two towers at a lower level) is returned whole.  Neither bound above holds there: |X| reaches Q/2,
// where k's estimate sits on its rounding boundary, and a k that is off by one leaves X -+ Q inside
// the 128-bit range.  The tables of such a tower set carry DeviceTables::crt_edge, and the launch takes
// crt_value's EDGE variant, which also flags the band of Q 2^-16 below Q/2 (build_ntt_tables measures
// the towers as this function does).  SHELFI_DEC_ALL_TOWERS=1 decodes with every tower (A/B probe
// switch; on chains too wide for crt_value's columns that is crt_exact_kernel).
static uint32_t decode_towers(const Params& p, uint32_t towers) {
  if (switches().dec_all_towers) return towers;
  uint32_t bits = 0;
  for (uint32_t t = 0; t < towers; ++t) {
    bits += 63 - (uint32_t)__builtin_clzll(p.q[t]);  // q_t >= 2^floor(log2 q_t)
    if (bits > 130) return t + 1;
  }
  return towers;
}

DecodePass decode_pass(shelfi_ctx* ctx, uint32_t towers, bool exact) {
  Params p = ctx->p;
  p.L = exact ? towers : decode_towers(ctx->p, towers);  // Q' = q_0 .. q_{p.L-1}; the secret key's first towers
  return DecodePass{p, p.L == ctx->p.L ? ctx->dt : level_q(ctx, p.L)};
}

}  // namespace shelfi

extern "C" {

int shelfi_set_decode_noise(shelfi_ctx* ctx, int enabled, double m_factor) {
  if (!ctx || !(m_factor >= 0.0) || !std::isfinite(m_factor)) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->decode_noise = enabled ? 1 : 0;
  ctx->decode_m_factor = m_factor;
  return SHELFI_OK;
}

int shelfi_set_slot_packing(shelfi_ctx* ctx, int mode) {
  if (!ctx) return SHELFI_ERR_ARG;
  if (mode != SHELFI_PACK_REAL && mode != SHELFI_PACK_COMPLEX) {
    set_error("slot packing: SHELFI_PACK_REAL (0) or SHELFI_PACK_COMPLEX (1)");
    return SHELFI_ERR_ARG;
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->p.pack = (uint32_t)mode;
  return SHELFI_OK;
}

int shelfi_get_slot_packing(const shelfi_ctx* ctx) {
  if (!ctx) return -1;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return (int)ctx->p.pack;
}

int shelfi_set_decode_exact(shelfi_ctx* ctx, int exact) {
  if (!ctx) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->decode_exact = exact ? 1 : 0;
  return SHELFI_OK;
}

int shelfi_decode_redo_count(shelfi_ctx* ctx, uint64_t* count) {
  if (!ctx || !count) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  *count = ctx->decode_redo_count;
  return SHELFI_OK;
}

int shelfi_encode_redo_count(shelfi_ctx* ctx, uint64_t* count) {
  if (!ctx || !count) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  *count = ctx->encode_redo_count;
  return SHELFI_OK;
}

int shelfi_decode_log_error(shelfi_ctx* ctx, int* log_error) {
  if (!ctx || !log_error) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    if (ctx->log_error_pending) {  // the last flooded decrypt's, read now (every call has synchronised)
      DeviceGuard g(ctx->device);
      SHELFI_HIP(hipMemcpy(ctx->host_flag + 2, ctx->dev_flag + 2, 4, hipMemcpyDeviceToHost));
      ctx->last_log_error = (int)ctx->host_flag[2];
      ctx->log_error_pending = false;
    }
    *log_error = ctx->last_log_error;
  });
}

}  // extern "C"
