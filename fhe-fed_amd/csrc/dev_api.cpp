// dev_api.cpp — the device API (shelfi_dev_*: device buffers in, device buffers out, the caller's
// stream): aggregation of separate batches, encrypt / decrypt and their threshold forms, the plaintext
// operands, and the evaluation calls (EvalMult, EvalInnerProduct, the Gram matrix, ModReduce, Rotate, EvalSum,
// EvalInnerProduct(ct, pt), EvalLinearWSum with encrypted weights, EvalPoly's combine, hoisted rotations, EvalAdd /
// Sub / Negate).  The packed resident arena is dev_arena.cpp.
#include <cmath>
#include <cstring>
#include <mutex>

#include "api_internal.h"
#include "api_util.h"
#include "eval_internal.h"

using namespace shelfi;

namespace shelfi {

// decrypt K ciphertexts of `towers` RNS towers (the context's L, or fewer after ModReduce)
// (sum_in: residues are uint64 sums of <= 16 canonical residues, folded on load; fuse: threshold
// fusion -- no ciphertexts and no key, the first pass sums fuse->P partial decryptions [K][towers][N]).
// The caller holds ctx->mu, has selected the device and checked the keys.
void dev_decrypt_locked(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, uint32_t towers, double scale, size_t n,
                        double* out_dev, hipStream_t s, bool sum_in, const FuseIn* fuse) {
  require_towers(ctx->p, towers);
  require_no_flood_on_complex(ctx);
  require_pair_aligned(ctx, out_dev);
  if (n > (uint64_t)K * values_per_ct(ctx->p)) throw Error{SHELFI_ERR_ARG, "n exceeds the slots in K ciphertexts"};
  const uint64_t Kn = (n + values_per_ct(ctx->p) - 1) / values_per_ct(ctx->p);
  if (!Kn) return;
  const size_t ct_words = 2ull * towers * ctx->p.N, part_words = (size_t)towers * ctx->p.N;
  const GenFlag fl = next_gen_flag(ctx);
  DecodeNoise dn = decode_noise_begin(ctx, Kn, fl);
  const uint64_t g0 = dn.g0;
  // one pass over the call: the decode's tower prefix with the fast CRT, or (exact) every tower
  // through crt_exact_kernel
  const auto run = [&](bool exact) {
    const DecodePass pass = decode_pass(ctx, towers, exact);
    const Params& p = pass.p;
    const DeviceTables& dt = pass.dt;
    dn.reset = 1;
    const auto bytes_of = [&](uint64_t kc) { return decrypt_scratch_bytes(p, kc); };
    for_chunks(ctx, Kn, switches().dev_chunk_mib, bytes_of, [&](uint64_t k0, uint64_t kc, void* scratch) {
      const uint64_t o0 = k0 * values_per_ct(p), on = std::min<uint64_t>(n - o0, kc * values_per_ct(p));
      dn.g0 = g0 + k0;
      if (fuse) {
        FuseIn fz = *fuse;
        for (uint32_t i = 0; i < fz.P; ++i) fz.part[i] += k0 * part_words;
        launch_decrypt(p, dt, ctx->dk, nullptr, kc, scale, on, out_dev + o0, scratch, s, &dn, false, towers, fl,
                       exact, &fz);
      } else {
        launch_decrypt(p, dt, ctx->dk, ct_dev + k0 * ct_words, kc, scale, on, out_dev + o0, scratch, s, &dn,
                       sum_in, towers, fl, exact);
      }
      dn.reset = 0;  // the flags are reset by the first chunk's flooding only
    });
    decode_noise_readback(ctx, dn);
  };
  // the wait after the last pass: scratch is reused by the next call
  decrypt_passes(ctx, fl, dn, run, [&] { SHELFI_HIP(hipStreamSynchronize(s)); });
}

static int dev_decrypt(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, uint32_t towers, double scale,
                       size_t n, double* out_dev, void* stream, bool sum_in = false) {
  if (!ctx || (n && (!ct_dev || !out_dev))) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    require_keys(ctx);
    DeviceGuard g(ctx->device);
    dev_decrypt_locked(ctx, ct_dev, K, towers, scale, n, out_dev, (hipStream_t)stream, sum_in, nullptr);
  });
}

// Partial decryption of K ciphertexts [K][2][towers][N] with the context's key share and smudging
// noise (threshold.hip); the noise stream advances by K.  The caller holds ctx->mu, has selected the
// device and checked the keys.  Synchronises s (the noise's scratch is reused by the next call).
void partial_decrypt_locked(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, uint32_t towers, bool lead,
                            uint64_t* out_dev, hipStream_t s) {
  const Params& p = ctx->p;
  require_towers(p, towers);
  if (!K) return;
  const double sigma = ctx->thr_sigma;
  uint32_t key[8] = {};
  KeyWiper wipe(key);
  const uint64_t g0 = ctx->thr_counter;
  ctx->thr_counter += K;
  if (sigma > 0.0) stream_key(ctx, key);
  const size_t tn = (size_t)towers * p.N;
  const auto launch = [&](uint64_t k0, uint64_t kc, void* scratch) {
    launch_partial_decrypt(p, ctx->dt, ctx->dk, ct_dev + k0 * 2 * tn, kc, towers, lead, out_dev + k0 * tn, scratch,
                           sigma, key, g0 + k0, s);
  };
  const size_t per_ct = partial_decrypt_scratch_bytes(p, towers, 1, sigma);
  if (!per_ct)  // sigma = 0: no noise, no scratch, one chain
    launch(0, K, nullptr);
  else
    for_chunks(ctx, K, switches().dev_chunk_mib, [&](uint64_t kc) { return per_ct * kc; }, launch);
  SHELFI_HIP(hipStreamSynchronize(s));
}

namespace {
// the key switch's scratch for a chain of K ciphertexts at the level of `a`
size_t ks_scratch(const KsArgs& a, uint32_t N, uint64_t K) {
  return ks_scratch_bytes(a.Ll, a.kP, a.dn, a.alpha, N, K);
}

// the three ciphertext-with-plaintext calls: op as launch_plain_op takes it
int dev_plain_op(int op, shelfi_ctx* ctx, const uint64_t* ct_dev, const uint64_t* pt_dev, size_t K, size_t Kp,
                 uint32_t towers, uint64_t* out_dev, void* stream) {
  if (!ctx || (K && (!ct_dev || !pt_dev || !out_dev))) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    const Params& p = ctx->p;
    require_towers(p, towers);
    if (!K) return;
    if (Kp != 1 && Kp != K) throw Error{SHELFI_ERR_ARG, "plaintext operand: one plaintext per ciphertext, or one for all"};
    // each thread reads its residues before writing them: out may be ct exactly, not shifted
    const uint64_t cw = 2ull * towers * p.N * K, pw = (uint64_t)towers * p.N * Kp;
    if (!out_exact_or_apart(out_dev, cw, {ct_dev}) || words_overlap(pt_dev, pw, out_dev, cw))
      throw Error{SHELFI_ERR_ARG, "plaintext operand: the output must be the ciphertext input exactly or overlap no input"};
    DeviceGuard g(ctx->device);
    launch_plain_op(op, ct_dev, pt_dev, K, Kp, towers, p.logN, ctx->dt.tc, out_dev, (hipStream_t)stream);
  });
}

// the three pointwise ciphertext calls: EvalAdd, EvalSub, and EvalNegate (no b_dev)
enum class CtOp { add, sub, negate };
int dev_ct_op(CtOp op, shelfi_ctx* ctx, const uint64_t* a_dev, const uint64_t* b_dev, size_t K, uint32_t towers,
              uint64_t* out_dev, void* stream) {
  if (!ctx || (K && (!a_dev || (op != CtOp::negate && !b_dev) || !out_dev))) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    const Params& p = ctx->p;
    require_towers(p, towers);
    if (!K) return;
    // each thread reads its residues before writing them: out may be an input exactly, not shifted
    const uint64_t words = 2ull * towers * p.N * K;
    if (!out_exact_or_apart(out_dev, words, {a_dev, b_dev}))
      throw Error{SHELFI_ERR_ARG, op == CtOp::add
                                      ? "EvalAdd output must be an input exactly or not overlap the inputs"
                                      : "EvalSub / EvalNegate output must be an input exactly or not overlap the inputs"};
    DeviceGuard g(ctx->device);
    (op == CtOp::add ? launch_ct_add : launch_ct_sub)(a_dev, b_dev, K * 2 * towers, towers, p.logN, ctx->dt.tc, out_dev,
                                                     (hipStream_t)stream);
  });
}

// Rotate's and Conjugate's call behind the key lookup: sigma_g and its key switch over K ciphertexts in launch
// chains under SHELFI_EVAL_CHUNK_MIB.  ctx lock held, device set.
void dev_galois_chains(shelfi_ctx* ctx, LevelState& l, const EvalState::RotKey& rk, uint32_t g, const uint64_t* ct_dev,
                       size_t K, uint32_t towers, uint64_t* out_dev, hipStream_t s, const char* overlap_msg) {
  const uint32_t N = ctx->p.N;
  const uint64_t ctw = 2ull * towers * N;
  if (!K) {
    ctx->eval_chunk_count = 0;
    return;
  }
  // the gather reads whole rows of the input while other workgroups write the output
  if (words_overlap(ct_dev, ctw * K, out_dev, ctw * K)) throw Error{SHELFI_ERR_ARG, overlap_msg};
  const KsArgs& a = l.args;
  const auto bytes_of = [&](uint64_t kc) { return ks_scratch(a, N, kc); };
  const uint64_t chains =
      for_chunks(ctx, K, switches().eval_chunk_mib, bytes_of, [&](uint64_t k0, uint64_t kc, void* scratch) {
        launch_rotate(a, ctx->dt, l.ext, l.dtf, rk.key, rk.key_sh, g, ct_dev + k0 * ctw, kc, out_dev + k0 * ctw,
                      scratch, s);
      });
  SHELFI_HIP(hipStreamSynchronize(s));  // scratch is reused by the next call
  ctx->eval_chunk_count = chains;
}
}  // namespace

}  // namespace shelfi

extern "C" {

int shelfi_dev_wavg(shelfi_ctx* ctx, const uint64_t* const* in_dev, const float* w, size_t C,
                    size_t K, uint64_t* out_dev, void* stream) {
  if (!ctx || !out_dev || (C && (!in_dev || !w))) return SHELFI_ERR_ARG;
  return guarded([&] {
    if (!C) throw Error{SHELFI_ERR_ARG, "no learners"};
    check_wavg_weights(w, C, ctx->p.delta);
    DeviceGuard g(ctx->device);
    const Params& p = ctx->p;
    hipStream_t s = (hipStream_t)stream;  // 0 = legacy default stream
    for (size_t c0 = 0; c0 < C; c0 += kWavgMaxLearners) {
      const size_t gc = std::min<size_t>(kWavgMaxLearners, C - c0);
      WavgArgs a;
      std::memset(&a, 0, sizeof(a));
      for (size_t c = 0; c < gc; ++c) a.ptrs[c] = in_dev[c0 + c];
      fill_weights(a, p, w + c0, gc);
      a.out = out_dev;
      a.rows = (uint64_t)K * 2 * p.L;
      a.C = (uint32_t)gc;
      a.L = p.L;
      a.logN = p.logN;
      a.accumulate = c0 ? 1 : 0;
      launch_wavg(a, ctx->dt.tc, s);
    }
  });
}

int shelfi_dev_check_residues(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, void* stream) {
  if (!ctx || (K && !ct_dev)) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    if (!K) return;
    DeviceGuard g(ctx->device);
    const Params& p = ctx->p;
    hipStream_t s = (hipStream_t)stream;
    uint32_t* bad = ctx->dev_flag + 6;
    SHELFI_HIP(hipMemsetAsync(bad, 0, 4, s));
    launch_check_residues(ct_dev, (uint64_t)K * 2 * p.L, p.L, p.logN, ctx->dt.tc, bad, s);
    SHELFI_HIP(hipMemcpyAsync(ctx->host_flag + 6, bad, 4, hipMemcpyDeviceToHost, s));
    SHELFI_HIP(hipStreamSynchronize(s));
    if (ctx->host_flag[6])
      throw Error{SHELFI_ERR_FORMAT, "ciphertext residue >= its tower modulus (malformed batch)"};
  });
}

int shelfi_dev_modq(shelfi_ctx* ctx, uint64_t* buf_dev, size_t K, void* stream) {
  if (!ctx || !buf_dev) return SHELFI_ERR_ARG;
  return guarded([&] {
    DeviceGuard g(ctx->device);
    hipStream_t s = (hipStream_t)stream;  // 0 = legacy default stream
    launch_modq(buf_dev, (uint64_t)K * 2 * ctx->p.L, ctx->p.L, ctx->p.logN, ctx->dt.tc, s);
  });
}

int shelfi_dev_encrypt(shelfi_ctx* ctx, const double* x_dev, size_t n, uint64_t* ct_dev,
                       void* stream) {
  if (!ctx || (n && (!x_dev || !ct_dev))) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    require_keys(ctx);
    DeviceGuard g(ctx->device);
    const Params& p = ctx->p;
    hipStream_t s = (hipStream_t)stream;  // 0 = legacy default stream
    const uint64_t K = (n + values_per_ct(p) - 1) / values_per_ct(p);
    if (!K) return;
    require_pair_aligned(ctx, x_dev);
    uint32_t key[8];
    KeyWiper wipe(key);
    uint64_t g0;
    draw_key(ctx, K, key, &g0);
    const GenFlag fl = next_gen_flag(ctx);
    const size_t ct_words = 2ull * p.L * p.N;
    // one pass over the call's chunks: the fast kernels, or (approx) the large-value path
    const auto bytes_of = [&](uint64_t kc) { return encrypt_scratch_bytes(p, kc); };
    const auto run = [&](bool approx) {
      for_chunks(ctx, K, switches().dev_chunk_mib, bytes_of, [&](uint64_t k0, uint64_t kc, void* scratch) {
        const uint64_t xs = k0 * values_per_ct(p), xn = std::min<uint64_t>(n - xs, kc * values_per_ct(p));
        uint64_t* ct = ct_dev + k0 * ct_words;
        if (approx)
          launch_encrypt_approx(p, ctx->dt, ctx->dk, x_dev + xs, xn, kc, ct, scratch, key, g0 + k0, s);
        else
          launch_encrypt(p, ctx->dt, ctx->dk, x_dev + xs, xn, kc, ct, scratch, key, g0 + k0, fl, s);
      });
    };
    run(false);
    SHELFI_HIP(hipStreamSynchronize(s));  // scratch is reused by the next call
    if (!encode_needs_approx(ctx, fl)) return;
    ++ctx->encode_redo_count;  // some message coefficient above 2^61: redo the call on the large-value path
    run(true);
  });
}

// ---- seeded ciphertexts (seeded.hip) ----
int shelfi_dev_encrypt_seeded(shelfi_ctx* ctx, const double* x_dev, size_t n, uint64_t* c0_dev, uint8_t seed_out[32],
                              void* stream) {
  if (!ctx || !seed_out || (n && (!x_dev || !c0_dev))) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    require_own_secret(ctx);
    DeviceGuard g(ctx->device);
    const Params& p = ctx->p;
    hipStream_t s = (hipStream_t)stream;
    const uint64_t K = (n + values_per_ct(p) - 1) / values_per_ct(p);
    require_pair_aligned(ctx, x_dev);
    uint32_t key[8], seed[8];
    KeyWiper wipe(key);
    uint64_t g0;
    draw_key(ctx, K, key, &g0);
    seeded_seed(key, g0, seed);
    std::memcpy(seed_out, seed, 32);
    if (!K) return;
    const GenFlag fl = next_gen_flag(ctx);
    const size_t c0_words = (size_t)p.L * p.N;
    const auto bytes_of = [&](uint64_t kc) { return seeded_encrypt_scratch_bytes(p, kc); };
    for_chunks(ctx, K, switches().dev_chunk_mib, bytes_of, [&](uint64_t k0, uint64_t kc, void* scratch) {
      const uint64_t xs = k0 * values_per_ct(p), xn = std::min<uint64_t>(n - xs, kc * values_per_ct(p));
      launch_encrypt_seeded(p, ctx->dt, ctx->dk, x_dev + xs, xn, kc, c0_dev + k0 * c0_words, scratch, key, g0 + k0,
                            seed, k0, fl, s);
    });
    SHELFI_HIP(hipStreamSynchronize(s));  // scratch is reused by the next call; the range words are final
    if (gen_flag_raised(ctx, fl, 1)) throw Error{SHELFI_ERR_RANGE, "encrypt_seeded: non-finite input value"};
    if (gen_flag_raised(ctx, fl, 0))
      throw Error{SHELFI_ERR_RANGE, "encrypt_seeded: a coefficient |x * scale| above 2^61 (the symmetric encrypt has no large-value path)"};
  });
}

int shelfi_dev_expand_seeded(shelfi_ctx* ctx, uint64_t* ct_dev, size_t K, uint32_t towers, const uint8_t seed[32],
                             uint64_t k0, void* stream) {
  if (!ctx || !seed || (K && !ct_dev)) return SHELFI_ERR_ARG;
  return guarded([&] {
    const Params& p = ctx->p;
    require_towers(p, towers);
    if (k0 >= kSeededMaxCts || K > kSeededMaxCts - k0)
      throw Error{SHELFI_ERR_ARG, "expand_seeded: ciphertext index at or above 2^48"};
    if (!K) return;
    DeviceGuard g(ctx->device);
    uint32_t sw[8];
    std::memcpy(sw, seed, 32);  // eight little-endian words
    launch_seeded_expand(sw, k0, K, towers, p.logN, ctx->dt.tc, ct_dev, (hipStream_t)stream);
  });
}

int shelfi_dev_decrypt(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, double scale, size_t n,
                       double* out_dev, void* stream) {
  return dev_decrypt(ctx, ct_dev, K, ctx ? ctx->p.L : 0, scale, n, out_dev, stream);
}

// ---- plaintext operands (plain.hip) ----
int shelfi_dev_encode(shelfi_ctx* ctx, const double* x_dev, size_t n, uint32_t towers, double scale,
                      uint64_t* pt_dev, void* stream) {
  if (!ctx || (n && (!x_dev || !pt_dev))) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    const Params& p = ctx->p;
    require_towers(p, towers);
    if (!(scale > 0.0) || !std::isfinite(scale)) throw Error{SHELFI_ERR_ARG, "encode: the scale must be finite and positive"};
    const uint64_t K = (n + values_per_ct(p) - 1) / values_per_ct(p);
    if (!K) return;
    require_pair_aligned(ctx, x_dev);
    DeviceGuard g(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    const GenFlag fl = next_gen_flag(ctx);  // the call's own generation of the range words
    const size_t pt_words = (size_t)towers * p.N;
    const auto bytes_of = [&](uint64_t kc) { return encode_scratch_bytes(p, kc); };
    for_chunks(ctx, K, switches().dev_chunk_mib, bytes_of, [&](uint64_t k0, uint64_t kc, void* scratch) {
      const uint64_t xs = k0 * values_per_ct(p), xn = std::min<uint64_t>(n - xs, kc * values_per_ct(p));
      launch_encode_plain(p, ctx->dt, x_dev + xs, xn, kc, towers, scale, pt_dev + k0 * pt_words, scratch, fl, s);
    });
    SHELFI_HIP(hipStreamSynchronize(s));  // scratch is reused by the next call; the range words are final
    if (gen_flag_raised(ctx, fl, 1)) throw Error{SHELFI_ERR_RANGE, "encode: non-finite input value"};
    if (gen_flag_raised(ctx, fl, 0))
      throw Error{SHELFI_ERR_RANGE, "encode: a coefficient |x * scale| above 2^61 (the plaintext encode has no large-value path)"};
  });
}

int shelfi_dev_mult_plain(shelfi_ctx* ctx, const uint64_t* ct_dev, const uint64_t* pt_dev, size_t K, size_t Kp,
                          uint32_t towers, uint64_t* out_dev, void* stream) {
  return dev_plain_op(0, ctx, ct_dev, pt_dev, K, Kp, towers, out_dev, stream);
}
int shelfi_dev_add_plain(shelfi_ctx* ctx, const uint64_t* ct_dev, const uint64_t* pt_dev, size_t K, size_t Kp,
                         uint32_t towers, uint64_t* out_dev, void* stream) {
  return dev_plain_op(1, ctx, ct_dev, pt_dev, K, Kp, towers, out_dev, stream);
}
int shelfi_dev_sub_plain(shelfi_ctx* ctx, const uint64_t* ct_dev, const uint64_t* pt_dev, size_t K, size_t Kp,
                         uint32_t towers, uint64_t* out_dev, void* stream) {
  return dev_plain_op(2, ctx, ct_dev, pt_dev, K, Kp, towers, out_dev, stream);
}
int shelfi_dev_add(shelfi_ctx* ctx, const uint64_t* a_dev, const uint64_t* b_dev, size_t K, uint32_t towers,
                   uint64_t* out_dev, void* stream) {
  return dev_ct_op(CtOp::add, ctx, a_dev, b_dev, K, towers, out_dev, stream);
}
int shelfi_dev_sub(shelfi_ctx* ctx, const uint64_t* a_dev, const uint64_t* b_dev, size_t K, uint32_t towers,
                   uint64_t* out_dev, void* stream) {
  return dev_ct_op(CtOp::sub, ctx, a_dev, b_dev, K, towers, out_dev, stream);
}
int shelfi_dev_negate(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, uint32_t towers, uint64_t* out_dev,
                      void* stream) {
  return dev_ct_op(CtOp::negate, ctx, ct_dev, nullptr, K, towers, out_dev, stream);
}

int shelfi_dev_decrypt_level(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, uint32_t towers, double scale,
                             size_t n, double* out_dev, void* stream) {
  return dev_decrypt(ctx, ct_dev, K, towers, scale, n, out_dev, stream);
}

int shelfi_dev_decrypt_sum(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, uint32_t terms, double scale,
                           size_t n, double* out_dev, void* stream) {
  if (terms < 1 || terms > (uint32_t)kMaxCommRanks) {
    set_error("decrypt_sum: the residues must be sums of 1..16 canonical residues");
    return SHELFI_ERR_ARG;
  }
  return dev_decrypt(ctx, ct_dev, K, ctx ? ctx->p.L : 0, scale, n, out_dev, stream, true);
}

int shelfi_dev_partial_decrypt(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, uint32_t towers, int lead,
                               uint64_t* out_dev, void* stream) {
  if (!ctx || (K && (!ct_dev || !out_dev))) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    require_keys(ctx);
    DeviceGuard g(ctx->device);
    partial_decrypt_locked(ctx, ct_dev, K, towers, lead != 0, out_dev, (hipStream_t)stream);
  });
}

int shelfi_dev_fuse_decrypt(shelfi_ctx* ctx, const uint64_t* const* partials_dev, size_t P, size_t K,
                            uint32_t towers, double scale, size_t n, double* out_dev, void* stream) {
  if (!ctx || (n && !out_dev)) return SHELFI_ERR_ARG;
  if (!partials_dev || P < 1 || P > (size_t)kMaxCommRanks) {
    set_error("fuse_decrypt: 1..16 partial decryptions");
    return SHELFI_ERR_ARG;
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    FuseIn fz{};
    fz.P = (uint32_t)P;
    for (size_t i = 0; i < P; ++i) {
      if (n && !partials_dev[i]) throw Error{SHELFI_ERR_ARG, "fuse_decrypt: null partial"};
      fz.part[i] = partials_dev[i];
    }
    DeviceGuard g(ctx->device);
    dev_decrypt_locked(ctx, nullptr, K, towers, scale, n, out_dev, (hipStream_t)stream, false, &fz);
  });
}

int shelfi_dev_ntt(shelfi_ctx* ctx, uint64_t* polys_dev, size_t P, int inverse, void* stream) {
  if (!ctx || (P && !polys_dev)) return SHELFI_ERR_ARG;
  return guarded([&] {
    DeviceGuard g(ctx->device);
    hipStream_t s = (hipStream_t)stream;  // 0 = legacy default stream
    launch_ntt(polys_dev, P, ctx->p.L, ctx->p.logN, inverse != 0, ctx->dt, s);
  });
}

// ---- the evaluation calls (keyswitch.hip, rotate.hip, hoist.hip): each cuts its K ciphertexts into
// launch chains under SHELFI_EVAL_CHUNK_MIB and leaves their number in ctx->eval_chunk_count ----
int shelfi_dev_mult(shelfi_ctx* ctx, const uint64_t* a_dev, const uint64_t* b_dev, size_t K, uint32_t towers,
                    uint64_t* out_dev, void* stream) {
  if (!ctx || (K && (!a_dev || !b_dev || !out_dev))) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    DeviceGuard g(ctx->device);
    if (!ctx->ev || !ctx->ev->evk)
      throw Error{SHELFI_ERR_STATE, "no evaluation key: call evalMultKeyGen() first"};
    LevelState& l = level(ctx, towers);
    if (!K) {
      ctx->eval_chunk_count = 0;
      return;
    }
    // out may alias a or b exactly (each workgroup reads its inputs before writing that
    // ciphertext's output); a shifted overlap would let one chunk's writes corrupt inputs
    // another has not read yet
    const uint32_t N = ctx->p.N;
    const uint64_t ctw = 2ull * towers * N;
    if (!out_exact_or_apart(out_dev, ctw * K, {a_dev, b_dev}))
      throw Error{SHELFI_ERR_ARG, "EvalMult output must be an input exactly or not overlap the inputs"};
    const KsArgs& a = l.args;
    hipStream_t s = (hipStream_t)stream;
    const auto bytes_of = [&](uint64_t kc) { return ks_scratch(a, N, kc); };
    const uint64_t chains =
        for_chunks(ctx, K, switches().eval_chunk_mib, bytes_of, [&](uint64_t k0, uint64_t kc, void* scratch) {
          launch_eval_mult(a, ctx->dt, l.ext, l.dtf, ctx->ev->evk, ctx->ev->evk_sh, a_dev + k0 * ctw, b_dev + k0 * ctw,
                           kc, out_dev + k0 * ctw, scratch, s);
        });
    SHELFI_HIP(hipStreamSynchronize(s));  // scratch is reused by the next call
    ctx->eval_chunk_count = chains;
  });
}

// EvalInnerProduct (dot.hip): one launch chain whatever K is -- the inputs are streamed, and the
// scratch holds the key switch of one ciphertext and at most 16 partial tensors
int shelfi_dev_dot(shelfi_ctx* ctx, const uint64_t* a_dev, const uint64_t* b_dev, size_t K, uint32_t towers,
                   uint64_t* out_dev, void* stream) {
  if (!ctx || !a_dev || !b_dev || !out_dev) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    DeviceGuard g(ctx->device);
    // a chain that cannot key-switch says so, before the key it can never hold is missed
    if (!eval_state(ctx).ks_error.empty()) throw Error{SHELFI_ERR_ARG, eval_state(ctx).ks_error};
    if (!ctx->ev || !ctx->ev->evk)
      throw Error{SHELFI_ERR_STATE, "no evaluation key: call evalMultKeyGen() first"};
    LevelState& l = level(ctx, towers);
    if (!K) throw Error{SHELFI_ERR_ARG, "EvalInnerProduct needs at least one ciphertext pair (an empty sum has no level)"};
    // the one output ciphertext is written while nothing says which input ciphertext it would replace: apart from both
    const uint32_t N = ctx->p.N;
    const uint64_t ctw = 2ull * towers * N;
    if (words_overlap(a_dev, ctw * K, out_dev, ctw) || words_overlap(b_dev, ctw * K, out_dev, ctw))
      throw Error{SHELFI_ERR_ARG, "EvalInnerProduct output must not overlap the inputs"};
    const KsArgs& a = l.args;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t S = dot_slices(K, switches().dot_slice_cts);
    void* scratch = ensure(ctx->scratch, ctx->scratch_bytes, dot_scratch_bytes(a, S));
    launch_dot(a, ctx->dt, l.ext, l.dtf, ctx->ev->evk, ctx->ev->evk_sh, a_dev, b_dev, K, S, out_dev, scratch, s);
    SHELFI_HIP(hipStreamSynchronize(s));  // scratch is reused by the next call
    ctx->dot_slice_count = S;
  });
}

uint64_t shelfi_dot_slice_count(const shelfi_ctx* ctx) {
  if (!ctx) return 0;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return ctx->dot_slice_count;
}

// The Gram matrix (gram.hip): the tiles of pairs cut into chains under SHELFI_EVAL_CHUNK_MIB, a
// chain the partial pass over its tiles, their reduction and one key switch of its pairs
int shelfi_dev_gram(shelfi_ctx* ctx, const uint64_t* const* batches_dev, size_t C, size_t K, uint32_t towers,
                    uint64_t* out_dev, void* stream) {
  if (!ctx || !batches_dev || !out_dev) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    if (C < 1 || C > (size_t)kGramMaxLearners) throw Error{SHELFI_ERR_ARG, "Gram needs 1..32 batches"};
    for (size_t i = 0; i < C; ++i)
      if (!batches_dev[i]) throw Error{SHELFI_ERR_ARG, "Gram: null batch"};
    DeviceGuard g(ctx->device);
    // a chain that cannot key-switch says so, before the key it can never hold is missed
    if (!eval_state(ctx).ks_error.empty()) throw Error{SHELFI_ERR_ARG, eval_state(ctx).ks_error};
    if (!ctx->ev || !ctx->ev->evk)
      throw Error{SHELFI_ERR_STATE, "no evaluation key: call evalMultKeyGen() first"};
    LevelState& l = level(ctx, towers);
    if (!K) throw Error{SHELFI_ERR_ARG, "Gram needs at least one ciphertext a batch (an empty sum has no level)"};
    // every input is read until the last chain's partial pass: the output lies apart from all of them
    const uint32_t N = ctx->p.N;
    const uint64_t ctw = 2ull * towers * N, P = gram_pairs(C);
    for (size_t i = 0; i < C; ++i)
      if (words_overlap(batches_dev[i], ctw * K, out_dev, ctw * P))
        throw Error{SHELFI_ERR_ARG, "Gram output must not overlap the inputs"};
    const KsArgs& a = l.args;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t S = gram_slices(C, K, a.Ll, a.logN, switches().gram_slice_cts);
    constexpr uint64_t tile_pairs = (uint64_t)kGramTile * kGramTile;  // (a diagonal or ragged tile holds fewer)
    const auto bytes_of = [&](uint64_t tc) { return gram_scratch_bytes(a, S, std::min(P, tc * tile_pairs)); };
    const uint64_t chains =
        for_chunks(ctx, gram_tiles(C), switches().eval_chunk_mib, bytes_of, [&](uint64_t t0, uint64_t tc, void* scratch) {
          launch_gram(a, ctx->dt, l.ext, l.dtf, ctx->ev->evk, ctx->ev->evk_sh, batches_dev, (uint32_t)C, t0, tc, K, S,
                      out_dev, scratch, s);
        });
    SHELFI_HIP(hipStreamSynchronize(s));  // scratch is reused by the next call
    ctx->eval_chunk_count = chains;
    ctx->gram_slice_count = S;
  });
}

size_t shelfi_gram_pairs(size_t C) { return (size_t)gram_pairs(C); }

uint64_t shelfi_gram_slice_count(const shelfi_ctx* ctx) {
  if (!ctx) return 0;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return ctx->gram_slice_count;
}

// EvalLinearWSum with encrypted weights (wsum.hip): the K output ciphertexts cut into chains under
// SHELFI_EVAL_CHUNK_MIB as shelfi_dev_mult's, a chain the summed-tensor pass over its share of every learner's
// batch and one key switch of its ciphertexts
int shelfi_dev_wsum_ct(shelfi_ctx* ctx, const uint64_t* const* batches_dev, size_t C, size_t K, uint32_t u_towers,
                       const uint64_t* const* weights_dev, size_t Kw, uint32_t towers, uint64_t* out_dev,
                       void* stream) {
  if (!ctx || !batches_dev || !weights_dev || !out_dev) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    if (C < 1 || C > (size_t)kWsumMaxLearners) throw Error{SHELFI_ERR_ARG, "EvalLinearWSum needs 1..32 learners"};
    for (size_t i = 0; i < C; ++i)
      if (!batches_dev[i] || !weights_dev[i]) throw Error{SHELFI_ERR_ARG, "EvalLinearWSum: null batch"};
    DeviceGuard g(ctx->device);
    // a chain that cannot key-switch says so, before the key it can never hold is missed
    if (!eval_state(ctx).ks_error.empty()) throw Error{SHELFI_ERR_ARG, eval_state(ctx).ks_error};
    if (!ctx->ev || !ctx->ev->evk)
      throw Error{SHELFI_ERR_STATE, "no evaluation key: call evalMultKeyGen() first"};
    if (towers < 1 || towers > u_towers || u_towers > ctx->p.L)
      throw Error{SHELFI_ERR_ARG, "EvalLinearWSum: 1 <= towers <= u_towers <= L (the updates sit at the weights' level or above)"};
    LevelState& l = level(ctx, towers);
    if (!K) throw Error{SHELFI_ERR_ARG, "EvalLinearWSum needs at least one update ciphertext a learner"};
    if (Kw != 1 && Kw != K)
      throw Error{SHELFI_ERR_ARG, "EvalLinearWSum: one weight ciphertext per update ciphertext, or one for all"};
    // every input is read by every chain's first pass: the output lies apart from all of them -- from an update
    // batch over the u_towers towers it is stored with, not only the ones read
    const uint32_t N = ctx->p.N;
    const uint64_t ctw = 2ull * towers * N, uctw = 2ull * u_towers * N;
    for (size_t i = 0; i < C; ++i)
      if (words_overlap(batches_dev[i], uctw * K, out_dev, ctw * K) ||
          words_overlap(weights_dev[i], ctw * Kw, out_dev, ctw * K))
        throw Error{SHELFI_ERR_ARG, "EvalLinearWSum output must not overlap the inputs"};
    const KsArgs& a = l.args;
    hipStream_t s = (hipStream_t)stream;
    const auto bytes_of = [&](uint64_t kc) { return ks_scratch(a, N, kc); };
    const uint64_t chains =
        for_chunks(ctx, K, switches().eval_chunk_mib, bytes_of, [&](uint64_t k0, uint64_t kc, void* scratch) {
          launch_wsum(a, ctx->dt, l.ext, l.dtf, ctx->ev->evk, ctx->ev->evk_sh, batches_dev, u_towers, weights_dev,
                      Kw == K && K > 1, (uint32_t)C, k0, kc, out_dev, scratch, s);
        });
    SHELFI_HIP(hipStreamSynchronize(s));  // scratch is reused by the next call
    ctx->eval_chunk_count = chains;
  });
}

// EvalPoly's combine (poly.hip): the constants go to the device through the context's table ring
// by a copy ordered on the stream; with giants the K outputs are cut into chains as shelfi_dev_wsum_ct's, a chain
// the summed-tensor pass over its share of every power and one key switch; without, one launch left enqueued
int shelfi_dev_poly_combine(shelfi_ctx* ctx, const uint64_t* const* babies_dev, const uint32_t* baby_towers,
                            uint32_t nb, const uint64_t* const* giants_dev, const uint32_t* giant_towers, uint32_t ng,
                            const uint64_t* table, size_t K, uint32_t towers, uint64_t* out_dev, void* stream) {
  if (!ctx || !babies_dev || !baby_towers || !table || !out_dev || (ng && (!giants_dev || !giant_towers)))
    return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    if (nb < 1 || nb > (uint32_t)kPolyMaxBabies) throw Error{SHELFI_ERR_ARG, "EvalPoly needs 1..3 baby-step powers"};
    if (ng > (uint32_t)kPolyMaxGiants) throw Error{SHELFI_ERR_ARG, "EvalPoly takes 0..7 giant-step powers"};
    for (uint32_t j = 0; j < nb; ++j)
      if (!babies_dev[j]) throw Error{SHELFI_ERR_ARG, "EvalPoly: null operand"};
    for (uint32_t g = 0; g < ng; ++g)
      if (!giants_dev[g]) throw Error{SHELFI_ERR_ARG, "EvalPoly: null operand"};
    DeviceGuard dg(ctx->device);
    const Params& p = ctx->p;
    if (ng) {
      // a chain that cannot key-switch says so, before the key it can never hold is missed
      if (!eval_state(ctx).ks_error.empty()) throw Error{SHELFI_ERR_ARG, eval_state(ctx).ks_error};
      if (!ctx->ev || !ctx->ev->evk)
        throw Error{SHELFI_ERR_STATE, "no evaluation key: call evalMultKeyGen() first"};
    }
    require_towers(p, towers);
    const auto stored = [&](uint32_t t) {
      if (t < towers || t > p.L)
        throw Error{SHELFI_ERR_ARG, "EvalPoly: towers <= an operand's towers <= L (every power sits at the combine level or above)"};
    };
    for (uint32_t j = 0; j < nb; ++j) stored(baby_towers[j]);
    for (uint32_t g = 0; g < ng; ++g) stored(giant_towers[g]);
    if (!K) throw Error{SHELFI_ERR_ARG, "EvalPoly needs at least one ciphertext"};
    // every operand is read by every chain's first pass: the output lies apart from all of them, over the towers
    // each is stored with, not only the ones read
    const uint32_t N = p.N;
    const uint64_t ctw = 2ull * towers * N;
    for (uint32_t j = 0; j < nb; ++j)
      if (words_overlap(babies_dev[j], 2ull * baby_towers[j] * N * K, out_dev, ctw * K))
        throw Error{SHELFI_ERR_ARG, "EvalPoly output must not overlap the operands"};
    for (uint32_t g = 0; g < ng; ++g)
      if (words_overlap(giants_dev[g], 2ull * giant_towers[g] * N * K, out_dev, ctw * K))
        throw Error{SHELFI_ERR_ARG, "EvalPoly output must not overlap the operands"};
    for (uint32_t g = 0; g <= ng; ++g)
      for (uint32_t j = 0; j <= nb; ++j)
        for (uint32_t t = 0; t < towers; ++t)
          if (table[((size_t)g * 4 + j) * towers + t] >= p.q[t])
            throw Error{SHELFI_ERR_ARG, "EvalPoly: a constant at or above its modulus"};
    LevelState* l = ng ? &level(ctx, towers) : nullptr;
    hipStream_t s = (hipStream_t)stream;
    // the constants as a workgroup reads them, [towers][ng + 1][4], written into the ring slot's own pinned words
    // (free once the slot is: the copy below is ordered before the kernels its event follows) and copied from
    // there, so the copy is a DMA the host does not wait for
    if (!ctx->poly_pin)
      SHELFI_HIP(hipHostMalloc((void**)&ctx->poly_pin, (size_t)shelfi_ctx::kWeightRing * kPolyTableWords * 8,
                               hipHostMallocDefault));
    const size_t wt_words = (size_t)towers * (ng + 1) * 4;
    const int slot = weight_ring_slot(ctx, wt_words * 8);
    uint64_t* wt = ctx->poly_pin + (size_t)slot * kPolyTableWords;
    for (uint32_t g = 0; g <= ng; ++g)
      for (uint32_t j = 0; j < 4; ++j)
        for (uint32_t t = 0; t < towers; ++t)
          wt[((size_t)t * (ng + 1) + g) * 4 + j] = j <= nb ? table[((size_t)g * 4 + j) * towers + t] : 0;
    SHELFI_HIP(hipMemcpyAsync(ctx->wl_dev[slot], wt, wt_words * 8, hipMemcpyHostToDevice, s));
    // the slot's event goes behind whatever was enqueued, also when a launch below throws: the ring waits for it
    // before it rewrites the slot
    struct SlotDone {
      hipEvent_t e;
      hipStream_t s;
      ~SlotDone() { (void)hipEventRecord(e, s); }
    } slot_done{ctx->wl_done[slot], s};
    const uint64_t* wt_dev = reinterpret_cast<const uint64_t*>(ctx->wl_dev[slot]);
    if (!ng) {
      launch_poly_combine(nullptr, ctx->dt, nullptr, nullptr, nullptr, nullptr, babies_dev, baby_towers, nb, nullptr,
                          nullptr, 0, wt_dev, towers, p.logN, 0, K, out_dev, nullptr, s);
      ctx->eval_chunk_count = 1;
      return;
    }
    const KsArgs& a = l->args;
    const auto bytes_of = [&](uint64_t kc) { return ks_scratch(a, N, kc); };
    const uint64_t chains =
        for_chunks(ctx, K, switches().eval_chunk_mib, bytes_of, [&](uint64_t k0, uint64_t kc, void* scratch) {
          launch_poly_combine(&a, ctx->dt, &l->ext, l->dtf, ctx->ev->evk, ctx->ev->evk_sh, babies_dev, baby_towers, nb,
                              giants_dev, giant_towers, ng, wt_dev, towers, p.logN, k0, kc, out_dev, scratch, s);
        });
    SHELFI_HIP(hipStreamSynchronize(s));  // scratch is reused by the next call
    ctx->eval_chunk_count = chains;
  });
}

// EvalInnerProduct(ct, pt) (dotp.hip): no key and one launch chain whatever C, R and K are -- the
// inputs are streamed; the slices' partial sums, when there are any, are held to the SHELFI_EVAL_CHUNK_MIB budget
int shelfi_dev_project(shelfi_ctx* ctx, const uint64_t* const* batches_dev, size_t C, const uint64_t* pts_dev,
                       size_t R, size_t K, uint32_t towers, uint64_t* out_dev, void* stream) {
  if (!ctx || !batches_dev || !pts_dev || !out_dev) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    if (C < 1 || C > (size_t)kDotpMaxBatches) throw Error{SHELFI_ERR_ARG, "EvalInnerProduct(ct, pt) needs 1..32 ciphertext batches"};
    if (R < 1 || R > (size_t)kDotpMaxBatches) throw Error{SHELFI_ERR_ARG, "EvalInnerProduct(ct, pt) needs 1..32 plaintext batches"};
    for (size_t i = 0; i < C; ++i)
      if (!batches_dev[i]) throw Error{SHELFI_ERR_ARG, "EvalInnerProduct(ct, pt): null batch"};
    const Params& p = ctx->p;
    require_towers(p, towers);
    if (!K) throw Error{SHELFI_ERR_ARG, "EvalInnerProduct(ct, pt) needs at least one ciphertext a batch (an empty sum has no level)"};
    // every input is read until the last workgroup ends: the output lies apart from all of them
    const uint64_t ptw = (uint64_t)towers * p.N, ctw = 2 * ptw, ow = ctw * C * R;
    bool apart = !words_overlap(pts_dev, ptw * K * R, out_dev, ow);
    for (size_t i = 0; i < C; ++i) apart = apart && !words_overlap(batches_dev[i], ctw * K, out_dev, ow);
    if (!apart) throw Error{SHELFI_ERR_ARG, "EvalInnerProduct(ct, pt) output must not overlap the inputs"};
    DeviceGuard g(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    const uint32_t S = dotp_slices(C, R, K, towers, p.logN, switches().dotp_slice_cts, switches().eval_chunk_mib << 20);
    void* scratch = S > 1 ? ensure(ctx->scratch, ctx->scratch_bytes, dotp_scratch_bytes(C, R, towers, p.logN, S)) : nullptr;
    launch_dotp(batches_dev, (uint32_t)C, pts_dev, (uint32_t)R, K, S, towers, p.logN, ctx->dt.tc, out_dev, scratch, s);
    if (S > 1) SHELFI_HIP(hipStreamSynchronize(s));  // scratch is reused by the next call
    ctx->dotp_slice_count = S;
  });
}

uint64_t shelfi_dotp_slice_count(const shelfi_ctx* ctx) {
  if (!ctx) return 0;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return ctx->dotp_slice_count;
}

int shelfi_dev_rescale(shelfi_ctx* ctx, const uint64_t* in_dev, size_t K, uint32_t towers, uint64_t* out_dev,
                       void* stream) {
  if (!ctx || (K && (!in_dev || !out_dev))) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    DeviceGuard g(ctx->device);
    const Params& p = ctx->p;
    if (towers < 2 || towers > p.L) throw Error{SHELFI_ERR_ARG, "ModReduce needs 2..L towers"};
    if (!K) {
      ctx->eval_chunk_count = 0;
      return;
    }
    const uint64_t in_ctw = 2ull * towers * p.N, out_ctw = 2ull * (towers - 1) * p.N;
    if (words_overlap(in_dev, in_ctw * K, out_dev, out_ctw * K))
      throw Error{SHELFI_ERR_ARG, "ModReduce input and output must not overlap"};
    RescaleConst rc{};
    rc.ql = p.q[towers - 1];
    for (uint32_t t = 0; t + 1 < towers; ++t) {
      rc.qlinv[t] = invmod(rc.ql % p.q[t], p.q[t]);
      rc.qlinv_sh[t] = shoup(rc.qlinv[t], p.q[t]);
    }
    hipStream_t s = (hipStream_t)stream;
    const auto bytes_of = [&](uint64_t kc) { return rescale_scratch_bytes(towers, p.N, kc); };
    const uint64_t chains =
        for_chunks(ctx, K, switches().eval_chunk_mib, bytes_of, [&](uint64_t k0, uint64_t kc, void* scratch) {
          launch_rescale(ctx->dt, towers, p.logN, rc, in_dev + k0 * in_ctw, kc, out_dev + k0 * out_ctw, scratch, s);
        });
    SHELFI_HIP(hipStreamSynchronize(s));
    ctx->eval_chunk_count = chains;
  });
}

int shelfi_dev_conjugate(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, uint32_t towers, uint64_t* out_dev,
                         void* stream) {
  if (!ctx || (K && (!ct_dev || !out_dev))) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    DeviceGuard dg(ctx->device);
    LevelState& l = level(ctx, towers);
    const uint32_t g = conjugation_galois(ctx->p.N);
    const EvalState::RotKey* rk = find_rot(ctx->ev, g);
    if (!rk) throw Error{SHELFI_ERR_STATE, "no conjugation key: call conjugateKeyGen() first"};
    dev_galois_chains(ctx, l, *rk, g, ct_dev, K, towers, out_dev, (hipStream_t)stream,
                      "conjugation input and output must not overlap");
  });
}

int shelfi_dev_rotate(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, uint32_t towers, int32_t index,
                      uint64_t* out_dev, void* stream) {
  if (!ctx || (K && (!ct_dev || !out_dev))) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    DeviceGuard dg(ctx->device);
    const uint32_t N = ctx->p.N;
    const uint32_t g = rotation_galois(ctx, index);
    hipStream_t s = (hipStream_t)stream;
    const uint64_t ctw = 2ull * towers * N;
    if (!index) {  // the identity: a copy (out may be the input itself)
      level_q(ctx, towers);
      if (K && out_dev != ct_dev) {
        if (words_overlap(ct_dev, ctw * K, out_dev, ctw * K))
          throw Error{SHELFI_ERR_ARG, "rotation input and output must not overlap"};
        SHELFI_HIP(hipMemcpyAsync(out_dev, ct_dev, ctw * K * 8, hipMemcpyDeviceToDevice, s));
        SHELFI_HIP(hipStreamSynchronize(s));
      }
      ctx->eval_chunk_count = 0;  // a copy: no launch chain
      return;
    }
    LevelState& l = level(ctx, towers);
    const EvalState::RotKey& rk = require_rot(ctx, index, g);
    dev_galois_chains(ctx, l, rk, g, ct_dev, K, towers, out_dev, s, "rotation input and output must not overlap");
  });
}

int shelfi_dev_rotate_many(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, uint32_t towers, const int32_t* indices,
                           size_t R, uint64_t* out_dev, void* stream) {
  if (!ctx || (R && !indices) || (K && R && (!ct_dev || !out_dev))) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    DeviceGuard dg(ctx->device);
    const uint32_t N = ctx->p.N;
    hipStream_t s = (hipStream_t)stream;
    const uint64_t ctw = 2ull * towers * N;
    require_towers(ctx->p, towers);
    if (R > kMaxRotKeys) throw Error{SHELFI_ERR_ARG, "rotate_many takes at most 64 rotations a call"};
    struct Rot {
      size_t r;  // its place in out
      uint32_t g, ginv;
      const EvalState::RotKey* rk;
    };
    std::vector<Rot> rots;  // every key is looked up before anything is enqueued
    std::vector<size_t> copies;
    bool have_level = false;
    for (size_t r = 0; r < R; ++r) {
      const uint32_t g = rotation_galois(ctx, indices[r]);
      if (!indices[r]) {
        copies.push_back(r);
        continue;
      }
      // a chain that cannot key-switch says so, before the keys it can never hold are missed
      if (!have_level) level(ctx, towers), have_level = true;
      rots.push_back(Rot{r, g, galois_element(N, -indices[r]), &require_rot(ctx, indices[r], g)});
    }
    ctx->eval_chunk_count = 0;
    if (!K || !R) return;
    if (words_overlap(ct_dev, ctw * K, out_dev, ctw * K * R))
      throw Error{SHELFI_ERR_ARG, "rotation input and output must not overlap"};
    level_q(ctx, towers);
    for (size_t r : copies)  // index 0: the input itself
      SHELFI_HIP(hipMemcpyAsync(out_dev + r * K * ctw, ct_dev, ctw * K * 8, hipMemcpyDeviceToDevice, s));
    uint64_t chains = 0;
    if (!rots.empty()) {
      LevelState& l = level(ctx, towers);
      const KsArgs& a = l.args;
      // rotations in flight behind one decomposition: as many accumulator sets as one ciphertext's share of the
      // budget holds beside the decomposition (at least one), so a long list splits over rotation groups
      // before a chain exceeds SHELFI_EVAL_CHUNK_MIB
      // (the floor, as chunk_split's: one ciphertext with one rotation in flight runs even when that alone is over
      // the budget -- include/shelfi.h says so)
      const uint64_t budget = (uint64_t)switches().eval_chunk_mib << 20;
      const uint64_t sh1 = hoist_shared_bytes(a, 1), acc1 = hoist_acc_bytes(a, 1);
      const uint64_t fit = budget > sh1 ? (budget - sh1) / acc1 : 0;
      const size_t Rg = (size_t)std::min<uint64_t>({rots.size(), (uint64_t)kHoistMaxGroup, std::max<uint64_t>(fit, 1)});
      const auto bytes_of = [&](uint64_t kc) { return hoist_shared_bytes(a, kc) + Rg * hoist_acc_bytes(a, kc); };
      const uint64_t kchains =
          for_chunks(ctx, K, switches().eval_chunk_mib, bytes_of, [&](uint64_t k0, uint64_t kc, void* scratch) {
            launch_hoist_decompose(a, ctx->dt, l.ext, l.dtf, ct_dev + k0 * ctw, kc, scratch, s);
            for (size_t i0 = 0; i0 < rots.size(); i0 += Rg) {
              HoistGroup grp{};
              grp.n = (uint32_t)std::min(Rg, rots.size() - i0);
              bool contiguous = kc == K;
              for (uint32_t i = 0; i < grp.n; ++i) {
                const Rot& rt = rots[i0 + i];
                grp.r[i] = HoistRot{rt.rk->key, rt.rk->key_sh, out_dev + (rt.r * K + k0) * ctw, rt.g, rt.ginv};
                contiguous = contiguous && rt.r == rots[i0].r + i;
              }
              launch_hoist_rotations(a, ctx->dt, l.ext, grp, contiguous, ct_dev + k0 * ctw, kc, scratch, s);
            }
          });
      chains = kchains * ((rots.size() + Rg - 1) / Rg);
    }
    SHELFI_HIP(hipStreamSynchronize(s));  // scratch is reused by the next call
    ctx->eval_chunk_count = chains;
  });
}

int shelfi_dev_eval_sum(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, uint32_t towers, uint32_t n,
                        uint64_t* out_dev, void* stream) {
  if (!ctx || (K && (!ct_dev || !out_dev))) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    DeviceGuard dg(ctx->device);
    const uint32_t N = ctx->p.N;
    if (!n || (n & (n - 1)) || n > ctx->p.batch)
      throw Error{SHELFI_ERR_ARG, "EvalSum needs a power of two in 1..batch"};
    hipStream_t s = (hipStream_t)stream;
    const uint64_t ctw = 2ull * towers * N;
    struct Step {
      uint32_t g;
      const EvalState::RotKey* rk;
    };
    std::vector<Step> steps;  // every key is looked up before anything is enqueued
    level_q(ctx, towers);
    // a chain that cannot key-switch says so, before the keys it can never hold are missed
    if (n > 1 && !eval_state(ctx).ks_error.empty()) throw Error{SHELFI_ERR_ARG, eval_state(ctx).ks_error};
    for (uint32_t r = 1; r < n; r <<= 1) {
      const uint32_t g = rotation_galois(ctx, (int32_t)r);
      steps.push_back(Step{g, &require_rot(ctx, (int32_t)r, g)});
    }
    if (!K) {
      ctx->eval_chunk_count = 0;
      return;
    }
    if (words_overlap(ct_dev, ctw * K, out_dev, ctw * K))
      throw Error{SHELFI_ERR_ARG, "EvalSum input and output must not overlap"};
    SHELFI_HIP(hipMemcpyAsync(out_dev, ct_dev, ctw * K * 8, hipMemcpyDeviceToDevice, s));
    uint64_t chains = 0;  // n = 1 is the copy alone
    if (!steps.empty()) {
      LevelState& l = level(ctx, towers);
      const KsArgs& a = l.args;
      // per chain: the key switch's scratch, rounded up to 64 bytes, then the rotated copy the accumulator takes in
      const auto ks_bytes = [&](uint64_t kc) { return (ks_scratch(a, N, kc) + 63) & ~(size_t)63; };
      const auto bytes_of = [&](uint64_t kc) { return ks_bytes(kc) + kc * ctw * 8; };
      chains = for_chunks(ctx, K, switches().eval_chunk_mib, bytes_of, [&](uint64_t k0, uint64_t kc, void* scratch) {
        uint64_t* rot = reinterpret_cast<uint64_t*>(static_cast<char*>(scratch) + ks_bytes(kc));
        uint64_t* acc = out_dev + k0 * ctw;
        for (const Step& st : steps) {
          launch_rotate(a, ctx->dt, l.ext, l.dtf, st.rk->key, st.rk->key_sh, st.g, acc, kc, rot, scratch, s);
          launch_ct_add(acc, rot, kc * 2 * towers, towers, ctx->p.logN, a.tq, acc, s);
        }
      });
    }
    SHELFI_HIP(hipStreamSynchronize(s));
    ctx->eval_chunk_count = chains;
  });
}

uint64_t shelfi_eval_chunk_count(const shelfi_ctx* ctx) {
  if (!ctx) return 0;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return ctx->eval_chunk_count;
}

}  // extern "C"
