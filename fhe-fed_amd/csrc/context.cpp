// context.cpp — the context's life behind the C ABI (include/shelfi.h): errors, key drawing, the
// NTT / CRT / FFT tables of a parameter set, keys and key files.
//
// Mirrors the reference's CKKS scheme wrapper, palisade_pybind/SHELFI_FHE/src/ckks.cpp:
//   shelfi_ctx_create        <- CKKS::CKKS                      (ckks.cpp:5-9)
//   shelfi_load              <- CKKS::loadCryptoParams          (ckks.cpp:11-23)
//   shelfi_keygen            <- CKKS::genCryptoContextAndKeyGen (ckks.cpp:25-59)
//   shelfi_encrypt           <- CKKS::encrypt                   (ckks.cpp:61-104)   bytes_api.cpp
//   shelfi_decrypt           <- CKKS::decrypt                   (ckks.cpp:170-213)  bytes_api.cpp
//   shelfi_weighted_average  <- CKKS::computeWeightedAverage    (ckks.cpp:264-320)  bytes_api.cpp
// Host code only validates, moves bytes and precomputes constant tables; every per-ciphertext
// operation is a kernel in one of the .hip files.
#include <sys/random.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <mutex>
#include <new>

#include "api_internal.h"
#include "api_util.h"
#include "palisade_codec.h"
#include "palisade_io.h"

using namespace shelfi;

namespace shelfi {

static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }

static uint64_t compute_params_id(const Params& p) {
  uint64_t h = fnv1a(&p.N, sizeof(p.N));
  h = fnv1a(&p.L, sizeof(p.L), h);
  return fnv1a(p.q, sizeof(uint64_t) * p.L, h);
}

static void seed_to_key(uint64_t seed, uint32_t key[8]) {
  uint64_t st = seed;
  for (int i = 0; i < 4; ++i) {
    uint64_t z = (st += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    key[2 * i] = (uint32_t)z;
    key[2 * i + 1] = (uint32_t)(z >> 32);
  }
}

static void os_random(void* buf, size_t n) {
  uint8_t* p = (uint8_t*)buf;
  while (n) {
    ssize_t r = getrandom(p, n, 0);
    if (r < 0) throw Error{SHELFI_ERR_DEVICE, "getrandom() failed"};
    p += r;
    n -= (size_t)r;
  }
}

void stream_key(const shelfi_ctx* ctx, uint32_t key[8]) {
  if (ctx->seed)
    seed_to_key(ctx->seed, key);
  else
    os_random(key, 32);
}

// encryption stream key + first ciphertext index for this call
void draw_key(shelfi_ctx* ctx, uint64_t count, uint32_t key[8], uint64_t* g0) {
  stream_key(ctx, key);
  *g0 = ctx->seed ? ctx->enc_counter : 0;
  if (ctx->seed) ctx->enc_counter += count;
}

// ------------------------------------------------------- tables / params ----
static void validate_params(uint32_t N, uint32_t L, uint32_t scale_bits, uint32_t first_mod_bits,
                            uint32_t batch) {
  if (L < 1 || L > (uint32_t)kMaxTowers) throw Error{SHELFI_ERR_ARG, "num_towers must be in [1,16]"};
  if (N < 1024 || N > (1u << 17) || (N & (N - 1)))
    throw Error{SHELFI_ERR_ARG, "ring dimension must be a power of two in [2^10, 2^17]"};
  if (!batch || (batch & (batch - 1)) || 2ull * batch > N)
    throw Error{SHELFI_ERR_ARG, "batchSize must be a power of two with 2*batchSize <= ring dimension"};
  if (scale_bits < 10 || scale_bits > 58)
    throw Error{SHELFI_ERR_ARG, "scaleFactorBits must be in [10, 58]"};
  if (first_mod_bits < scale_bits || first_mod_bits > 60)
    throw Error{SHELFI_ERR_ARG, "firstModBits must be in [scaleFactorBits, 60]"};
}

// Little-endian 30-bit limbs (the decode CRT's tables): the product of q[0..L) (except q[skip]), its
// two's-complement negation, mod 2^(30 n).
static std::vector<uint64_t> mw30_mul(std::vector<uint64_t> a, uint64_t m) {
  u128 carry = 0;
  for (auto& x : a) {
    const u128 v = (u128)x * m + carry;
    x = (uint64_t)v & ((1u << 30) - 1);
    carry = v >> 30;
  }
  return a;
}
static std::vector<uint64_t> mw30_qhat(const uint64_t* q, uint32_t L, uint32_t skip, uint32_t n) {
  std::vector<uint64_t> a(n, 0);
  a[0] = 1;
  for (uint32_t u = 0; u < L; ++u)
    if (u != skip) a = mw30_mul(std::move(a), q[u]);
  return a;
}
static std::vector<uint64_t> mw30_prod(const uint64_t* q, uint32_t L, uint32_t n) {
  return mw30_qhat(q, L, L, n);
}
static std::vector<uint64_t> mw30_neg(std::vector<uint64_t> a, uint32_t n) {
  uint64_t carry = 1;
  for (uint32_t j = 0; j < n; ++j) {
    const uint64_t v = ((~a[j]) & ((1u << 30) - 1)) + carry;
    a[j] = v & ((1u << 30) - 1);
    carry = v >> 30;
  }
  return a;
}

void free_ntt_tables(DeviceTables& dt) {
  dfree_t(dt.crt_mw);
  dt.crt_nc = 0;
  dt.crt_edge = false;
  dfree_t(dt.tc);
  dfree_t(dt.psi_rev);
  dfree_t(dt.psi_rev_sh);
  dfree_t(dt.ipsi_rev);
  dfree_t(dt.ipsi_rev_sh);
  dfree_t(dt.tw_fwd_blk);
  dfree_t(dt.tw_inv_blk);
}

static void free_tables(shelfi_ctx* ctx) {
  eval_release(ctx, false);  // level / extended-basis tables belong to these parameters
  ctx->arena_refused.clear();  // arenas are laid out for these parameters
  free_ntt_tables(ctx->dt);
  dfree_t(ctx->dt.fft_inv);
  dfree_t(ctx->dt.fft_fwd);
  dfree_t(ctx->dt.cdt);
  dfree_t(ctx->dt.enc_tab);
  dfree_t(ctx->dt.enc_vtab);
}

static void free_keys(shelfi_ctx* ctx) {
  eval_release(ctx, true);  // the relinearization key belongs to the secret key
  ctx->arena_refused.clear();  // a reload starts a new parameter/key generation of arenas
  dfree_t(ctx->dk.pk);
  dfree_t(ctx->dk.pk_sh);
  dfree_t(ctx->dk.sk);
  dfree_t(ctx->dk.sk_sh);
  ctx->keys_loaded = false;
  ctx->key_id = 0;
  ctx->pk_host.clear();
  ctx->sk_host.clear();
}

static uint32_t bitrev_host(uint32_t x, uint32_t bits) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < bits; ++i) r = (r << 1) | ((x >> i) & 1);
  return r;
}

// NTT / CRT tables of the towers p.q[0..L) (the context's chain, one of its levels, or an
// extended basis Q_l u P of the key switching in eval_state.cpp).
void build_ntt_tables(const Params& p, DeviceTables& dt) {
  free_ntt_tables(dt);
  const uint32_t N = p.N, L = p.L;
  std::vector<TowerConst> tc(L);
  std::vector<uint64_t> pr((size_t)L * N), prs((size_t)L * N), ipr((size_t)L * N), iprs((size_t)L * N);
  for (uint32_t t = 0; t < L; ++t) {
    const uint64_t q = p.q[t];
    TowerConst& c = tc[t];
    std::memset(&c, 0, sizeof(c));
    c.q = q;
    c.one_shoup = (uint64_t)(((u128)1 << 64) / q);
    c.r30 = (1ull << 30) % q;
    c.r30_shoup = shoup(c.r30, q);
    c.r60 = (1ull << 60) % q;
    c.r60_shoup = shoup(c.r60, q);
    c.r64 = (uint64_t)(((u128)1 << 64) % q);
    c.r64_shoup = shoup(c.r64, q);
    c.ninv = invmod(N % q, q);
    c.ninv_shoup = shoup(c.ninv, q);
    uint64_t qhat_mod = 1;
    for (uint32_t u = 0; u < L; ++u)
      if (u != t) qhat_mod = (uint64_t)(((u128)qhat_mod * (p.q[u] % q)) % q);
    c.qhat_inv = invmod(qhat_mod, q);
    c.qhat_inv_shoup = shoup(c.qhat_inv, q);
    c.ninv_qhat = (uint64_t)(((u128)c.ninv * c.qhat_inv) % q);
    c.ninv_qhat_shoup = shoup(c.ninv_qhat, q);
    {
      const std::vector<uint64_t> qh = mw30_qhat(p.q, L, t, 7), nq = mw30_neg(mw30_prod(p.q, L, 7), 7);
      for (int j = 0; j < 7; ++j) {
        c.crt30[j] = (uint32_t)qh[j];
        c.nq30[j] = (uint32_t)nq[j];
      }
    }
    c.inv_q = 1.0 / (double)q;
    c.nq = (uint64_t)0 - q;
    c.n4q = (uint64_t)0 - (q << 2);
    c.n8q = (uint64_t)0 - (q << 3);
    {
      const uint32_t E = 63 - (uint32_t)__builtin_clzll(q);  // 2^E <= q < 2^(E+1)
      c.red_ok = E >= 40;
      c.red_sh = E >= 32 ? E - 32 : 0;
      c.red_r = c.red_ok ? (uint32_t)(((u128)1 << (32 + E)) / q) : 0;
      c.crt_sh = E >= 31 ? E - 31 : 0;
      c.bq62 = ((1ull << 62) / q) * q;
      c.bmu = E <= 59 ? (uint64_t)(((u128)1 << (2 * E + 2)) / q) : 0;  // plain_mulmod takes q < 2^60
      c.inv_q32 = (float)((double)(1ull << c.crt_sh) / (double)q);
    }
    // twiddles: psi^bitrev(i), psi^-bitrev(i)
    const uint64_t ipsi = invmod(p.psi[t], q);
    uint64_t a = 1, b = 1;
    for (uint32_t i = 0; i < N; ++i) {
      const uint32_t r = bitrev_host(i, p.logN);
      pr[(size_t)t * N + r] = a;
      ipr[(size_t)t * N + r] = b;
      a = (uint64_t)(((u128)a * p.psi[t]) % q);
      b = (uint64_t)(((u128)b * ipsi) % q);
    }
    for (uint32_t i = 0; i < N; ++i) {
      prs[(size_t)t * N + i] = shoup(pr[(size_t)t * N + i], q);
      iprs[(size_t)t * N + i] = shoup(ipr[(size_t)t * N + i], q);
    }
    c.ninv_qhat_w1 = (uint64_t)(((u128)c.ninv_qhat * ipr[(size_t)t * N + 1]) % q);
    c.ninv_qhat_w1_shoup = shoup(c.ninv_qhat_w1, q);
  }
  {
    // decode's CRT (DeviceTables::crt_nc / crt_mw): |sum_t y_t Q/q_t - k Q| < L Q, plus a sign bit
    uint32_t qbits = 0;
    for (uint32_t t = 0; t < L; ++t) qbits += 64 - (uint32_t)__builtin_clzll(p.q[t]);
    const uint32_t need = qbits + (32 - (uint32_t)__builtin_clz(L)) + 1;
    const uint32_t nc = std::max<uint32_t>(5, (need + 29) / 30);
    dt.crt_nc = (L <= 7 && nc <= 7) ? nc : 0;
    const uint32_t NL = (need + 1 + 29) / 30, NW = (qbits + 63) / 64 + 1;
    if (NL > (uint32_t)kCrtMwMaxLimbs) throw Error{SHELFI_ERR_ARG, "tower chain too wide for the exact CRT"};
    std::vector<uint32_t> mw(4 + (size_t)(L + 2) * NL, 0);
    mw[0] = NL;
    mw[1] = NW;
    const std::vector<uint64_t> Qm = mw30_prod(p.q, L, NL), nQ = mw30_neg(Qm, NL);
    for (uint32_t t = 0; t < L; ++t) {
      const std::vector<uint64_t> qh = mw30_qhat(p.q, L, t, NL);
      for (uint32_t j = 0; j < NL; ++j) mw[4 + (size_t)t * NL + j] = (uint32_t)qh[j];
    }
    for (uint32_t j = 0; j < NL; ++j) {
      mw[4 + (size_t)L * NL + j] = (uint32_t)nQ[j];
      // (Q - 1) / 2 = Q >> 1 (Q odd)
      mw[4 + (size_t)(L + 1) * NL + j] = (uint32_t)((Qm[j] >> 1) | (j + 1 < NL ? (Qm[j + 1] & 1) << 29 : 0));
    }
    dt.crt_mw = upload(mw.data(), mw.size());
    // A chain at or below 2^130 (decode_towers' measure) is decoded whole by the fast path: the
    // launch flags |X'| >= (Q - 1) / 2 - floor(Q 2^-16) as well (TowerConst::crt_edge).  Such a Q is
    // below 2^(130 + L), three 64-bit words.
    uint32_t fbits = 0;
    for (uint32_t t = 0; t < L; ++t) fbits += 63 - (uint32_t)__builtin_clzll(p.q[t]);
    dt.crt_edge = dt.crt_nc != 0 && fbits <= 130;
    if (dt.crt_edge) {
      uint64_t Qw[3] = {0, 0, 0};
      for (uint32_t j = 0; j < NL && 30 * j < 192; ++j) {
        Qw[30 * j / 64] |= Qm[j] << (30 * j % 64);
        if (30 * j % 64 > 34 && 30 * j / 64 + 1 < 3) Qw[30 * j / 64 + 1] |= Qm[j] >> (64 - 30 * j % 64);
      }
      const auto shr = [&](uint32_t s, uint64_t* o) {  // o = Q >> s, 0 < s < 64
        for (int w = 0; w < 3; ++w) o[w] = (Qw[w] >> s) | (w + 1 < 3 ? Qw[w + 1] << (64 - s) : 0);
      };
      uint64_t h[3], m[3], e[3];
      shr(1, h);
      shr(16, m);
      uint64_t borrow = 0;
      for (int w = 0; w < 3; ++w) {
        const u128 d = (u128)h[w] - m[w] - borrow;
        e[w] = (uint64_t)d;
        borrow = (uint64_t)(d >> 64) & 1;
      }
      const bool past = e[2] != 0 || (e[1] >> 63) != 0;  // 2^127 or more: the 128-bit range test covers it
      for (uint32_t t = 0; t < L; ++t) {
        tc[t].crt_edge[0] = past ? ~0ull : e[0];
        tc[t].crt_edge[1] = past ? ~0ull : e[1];
      }
    }
  }
  dt.tc = upload(tc.data(), L);
  dt.red_ok = true;
  for (uint32_t t = 0; t < L; ++t) dt.red_ok = dt.red_ok && tc[t].red_ok;
  dt.psi_rev = upload(pr.data(), pr.size());
  dt.psi_rev_sh = upload(prs.data(), prs.size());
  dt.ipsi_rev = upload(ipr.data(), ipr.size());
  dt.ipsi_rev_sh = upload(iprs.data(), iprs.size());
  {
    // per-block twiddle slices: entry 2^l + i of block b = psi table index
    // 2^(sstart + l) + b 2^l + i (local stage l of a 2^BL-element block)
    auto slices = [&](uint32_t BL, const std::vector<uint64_t>& w, const std::vector<uint64_t>& ws) {
      const uint32_t sstart = p.logN - BL;
      std::vector<ulonglong2> out((size_t)L * N);
      for (uint32_t t = 0; t < L; ++t)
        for (uint32_t b = 0; b < (1u << sstart); ++b) {
          const size_t base = (size_t)t * N + ((size_t)b << BL);
          out[base] = make_ulonglong2(0, 0);
          for (uint32_t l = 0; l < BL; ++l)
            for (uint32_t i = 0; i < (1u << l); ++i) {
              const size_t src = (size_t)t * N + (1ull << (sstart + l)) + ((size_t)b << l) + i;
              out[base + (1u << l) + i] = make_ulonglong2(w[src], ws[src]);
            }
        }
      return out;
    };
    const uint32_t BL = ntt_block_log(p.logN);
    dt.tw_fwd_blk = upload(slices(BL, pr, prs).data(), (size_t)L * N);
    dt.tw_inv_blk = upload(slices(BL, ipr, iprs).data(), (size_t)L * N);
  }
}

// (Re)build every device table for ctx->p.
static void build_tables(shelfi_ctx* ctx) {
  free_tables(ctx);
  Params& p = ctx->p;
  build_ntt_tables(p, ctx->dt);
  const uint32_t S = p.batch;
  std::vector<double> ir(S), ii(S), fr(S), fi(S);
  fft_twiddles(S, ir.data(), ii.data(), fr.data(), fi.data());
  std::vector<double2> tinv(S), tfwd(S);
  for (uint32_t i = 0; i < S; ++i) {
    tinv[i] = make_double2(ir[i], ii[i]);
    tfwd[i] = make_double2(fr[i], fi[i]);
  }
  ctx->dt.fft_inv = upload(tinv.data(), S);
  ctx->dt.fft_fwd = upload(tfwd.data(), S);
  uint64_t cdt[64];
  // <= 63 entries: the samplers' 6-step binary search over the 64-padded table counts
  // at most 63 (sigma <= 4.77; the default 3.19 gives 43)
  ctx->dt.cdt_len = gauss_cdt(p.sigma, cdt, 63);
  if (ctx->dt.cdt_len < 0) throw Error{SHELFI_ERR_ARG, "Gaussian table too large"};
  ctx->dt.cdt = upload(cdt, (size_t)ctx->dt.cdt_len);
  // enc_cols_fused's small-polynomial tables: the columns pass's first twiddles are
  // psi_rev[1] = psi^(N/2) (stage 0) and psi_rev[2], psi_rev[3] = psi^(N/4), psi^(3N/4) (stage 1)
  {
    std::vector<uint64_t> et((size_t)p.L * kEncTab);
    for (uint32_t t = 0; t < p.L; ++t) {
      const uint64_t q = p.q[t];
      const uint64_t W0 = powmod(p.psi[t], p.N / 2, q), W1 = powmod(p.psi[t], p.N / 4, q),
                     W2 = powmod(p.psi[t], 3ull * p.N / 4, q);
      const auto mul = [q](uint64_t a, uint64_t b) { return (uint64_t)(((u128)a * b) % q); };
      const auto sm = [q](int v) { return v < 0 ? q - (uint64_t)(-v) : (uint64_t)v; };  // |v| < q
      const auto add = [q](uint64_t a, uint64_t b) { return (uint64_t)(((u128)a + b) % q); };
      const auto sub = [q](uint64_t a, uint64_t b) { return a >= b ? a - b : a + q - b; };
      uint64_t* T = et.data() + (size_t)t * kEncTab;
      for (int idx = 0; idx < 81; ++idx) {
        const uint64_t a = sm(idx % 3 - 1), b = sm(idx / 3 % 3 - 1), c = sm(idx / 9 % 3 - 1), d = sm(idx / 27 - 1);
        const uint64_t u = add(a, mul(W0, c)), v = add(b, mul(W0, d));  // stage 0 (pairs a-c, b-d)
        const uint64_t u2 = sub(a, mul(W0, c)), v2 = sub(b, mul(W0, d));
        T[0 * 81 + idx] = add(u, mul(W1, v));  // stage 1 (pairs a'-b' with W1, c'-d' with W2)
        T[1 * 81 + idx] = sub(u, mul(W1, v));
        T[2 * 81 + idx] = add(u2, mul(W2, v2));
        T[3 * 81 + idx] = sub(u2, mul(W2, v2));
      }
      for (int e = -64; e < 64; ++e) {
        const uint64_t m = mul(W0, sm(e < 0 ? -e : e));
        T[kEncVTab + 64 + e] = e < 0 ? (m ? q - m : 0) : m;
      }
    }
    ctx->dt.enc_tab = upload(et.data(), et.size());
  }
  // NTT(v)'s 4 column stages as table sums (DeviceTables::enc_vtab): the stages' 16 x 16 matrix M_t
  // (row r' of the output from input row r, the columns pass's twiddles psi_rev[m + i] at stage
  // s = log2 m) applied to the ternary rows of each group g = {g, g + 4, g + 8, g + 12}
  if (p.logN >= 15 && p.logN - ntt_block_log(p.logN) == 4) {
    constexpr int R = 16;
    std::vector<uint64_t> vt((size_t)p.L * R * 4 * 81);
    for (uint32_t t = 0; t < p.L; ++t) {
      const uint64_t q = p.q[t];
      const auto mul = [q](uint64_t a, uint64_t b) { return (uint64_t)(((u128)a * b) % q); };
      const auto add = [q](uint64_t a, uint64_t b) { return (uint64_t)(((u128)a + b) % q); };
      const auto sub = [q](uint64_t a, uint64_t b) { return a >= b ? a - b : a + q - b; };
      // psi_rev[m + i] = psi^bitrev_logN(m + i)
      const auto tw = [&](uint32_t idx) { return powmod(p.psi[t], bitrev_host(idx, p.logN), q); };
      uint64_t M[R][R];  // M[r'][r]
      for (int r = 0; r < R; ++r) {
        uint64_t x[R] = {0};
        x[r] = 1;
        for (int s = 0; s < 4; ++s) {
          const int m = 1 << s, tr = R >> (s + 1);
          for (int i = 0; i < m; ++i) {
            const uint64_t W = tw((uint32_t)(m + i));
            for (int jj = 0; jj < tr; ++jj) {
              const int r0 = 2 * i * tr + jj, r1 = r0 + tr;
              const uint64_t a = x[r0], b = mul(W, x[r1]);
              x[r0] = add(a, b);
              x[r1] = sub(a, b);
            }
          }
        }
        for (int rp = 0; rp < R; ++rp) M[rp][r] = x[rp];
      }
      for (int rp = 0; rp < R; ++rp)
        for (int g = 0; g < 4; ++g)
          for (int idx = 0; idx < 81; ++idx) {
            uint64_t acc = 0;
            for (int kk = 0, d = idx; kk < 4; ++kk, d /= 3) {
              const int trit = d % 3 - 1;
              const uint64_t e = M[rp][g + 4 * kk];
              acc = trit > 0 ? add(acc, e) : trit < 0 ? sub(acc, e) : acc;
            }
            vt[(((size_t)t * R + rp) * 4 + g) * 81 + idx] = acc;
          }
    }
    ctx->dt.enc_vtab = upload(vt.data(), vt.size());
  }
  ctx->params_id = compute_params_id(p);
}

static void set_params(shelfi_ctx* ctx, uint32_t N, uint32_t L, uint32_t scale_bits,
                       uint32_t first_mod_bits, uint32_t batch, const uint64_t* q,
                       const uint64_t* psi) {
  Params p;
  p.N = N;
  p.logN = (uint32_t)__builtin_ctz(N);
  p.L = L;
  p.batch = batch;
  p.gap = N / (2 * batch);
  p.scale_bits = scale_bits;
  p.first_mod_bits = first_mod_bits;
  for (uint32_t t = 0; t < L; ++t) {
    if (q[t] >= (1ull << 60) || q[t] % (2ull * N) != 1)
      throw Error{SHELFI_ERR_ARG, "modulus out of range (need q < 2^60, q = 1 mod 2N)"};
    if (powmod(psi[t], N, q[t]) != q[t] - 1)
      throw Error{SHELFI_ERR_ARG, "root of unity is not a primitive 2N-th root"};
    p.q[t] = q[t];
    p.psi[t] = psi[t];
  }
  // EXACTRESCALE level-0 scaling factor = (double)q_{L-1} (CT1.txt@265059).
  p.delta = (double)q[L - 1];
  p.pack = ctx->p.pack;  // context state (shelfi_set_slot_packing), kept across a parameter reload
  ctx->p = p;
  build_tables(ctx);
}

// keys: host copies -> device (+ Shoup companions)
static void install_keys(shelfi_ctx* ctx, const uint64_t* pk, const uint64_t* sk, bool palisade) {
  const Params& p = ctx->p;
  const size_t LN = (size_t)p.L * p.N;
  for (size_t i = 0; i < 2 * LN; ++i)
    if (pk[i] >= p.q[(i / p.N) % p.L]) throw Error{SHELFI_ERR_FORMAT, "public key residue >= q"};
  for (size_t i = 0; i < LN; ++i)
    if (sk[i] >= p.q[i / p.N]) throw Error{SHELFI_ERR_FORMAT, "secret key residue >= q"};
  free_keys(ctx);
  std::vector<uint64_t> pks(2 * LN), sks(LN);
  for (size_t i = 0; i < 2 * LN; ++i) pks[i] = shoup(pk[i], p.q[(i / p.N) % p.L]);
  for (size_t i = 0; i < LN; ++i) sks[i] = shoup(sk[i], p.q[i / p.N]);
  ctx->dk.pk = upload(pk, 2 * LN);
  ctx->dk.pk_sh = upload(pks.data(), 2 * LN);
  ctx->dk.sk = upload(sk, LN);
  ctx->dk.sk_sh = upload(sks.data(), LN);
  ctx->pk_host.assign(pk, pk + 2 * LN);
  ctx->sk_host.assign(sk, sk + LN);
  ctx->key_id = fnv1a(pk, sizeof(uint64_t) * 2 * LN, ctx->params_id);
  ctx->keys_loaded = true;
  ctx->threshold_share = false;  // shelfi_multiparty_keygen raises it again after its install
  ctx->palisade_keys = palisade;
  if (!palisade) {  // PALISADE wire format needs the PALISADE context + key tag
    ctx->pal_ctx_obj.clear();
    ctx->pal_keytag.clear();
    ctx->wire = 0;
  }
}

void require_keys(const shelfi_ctx* ctx) {
  if (!ctx->keys_loaded)
    throw Error{SHELFI_ERR_STATE,
                "no keys: call loadCryptoParams() or genCryptoContextAndKeyGen() first"};
}

// The symmetric (seeded) encrypt: a ciphertext under one party's share of a threshold key is not a
// ciphertext under the joint key.
void require_own_secret(const shelfi_ctx* ctx) {
  require_keys(ctx);
  if (ctx->threshold_share)
    throw Error{SHELFI_ERR_STATE, "seeded encryption needs the whole secret key: this context holds a threshold share (multipartyKeyGen)"};
}

// -------------------------------------------------- own key-file format ----
// cryptocontext.txt: "SHCC" u32 version, u32 N, L, batch, scale_bits, first_mod_bits,
//                    f64 sigma, u64 q[L], u64 psi[L]
// key-public.txt:    "SHPK" u32 version, u64 params_id, u64 [2][L][N]
// key-private.txt:   "SHSK" u32 version, u64 params_id, u64 [L][N]
static void write_file(const std::string& path, const std::string& data) {
  std::ofstream f(path, std::ios::binary | std::ios::trunc);
  if (!f) throw Error{SHELFI_ERR_IO, "cannot open " + path + " for writing"};
  f.write(data.data(), (std::streamsize)data.size());
  if (!f) throw Error{SHELFI_ERR_IO, "error writing " + path};
}
static std::string read_file(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw Error{SHELFI_ERR_IO, "could not read " + path};
  return std::string((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
template <class T>
static void put(std::string& s, const T& v) {
  s.append(reinterpret_cast<const char*>(&v), sizeof(T));
}
template <class T>
static T get(const std::string& s, size_t& off) {
  if (off + sizeof(T) > s.size()) throw Error{SHELFI_ERR_FORMAT, "truncated key file"};
  T v;
  std::memcpy(&v, s.data() + off, sizeof(T));
  off += sizeof(T);
  return v;
}

// PALISADE context parameters of ctx->p, as genCryptoContextCKKS(multDepth, scaleFactorBits,
// batchSize) records them (ckks.cpp:28): the scaling-factor bits in the plaintext-modulus
// field, the batch in the encoding parameters, the default RLWE fields of the reference's
// committed cryptocontext.txt.
static PalisadeCtxParams palisade_params_of(const Params& p) {
  PalisadeCtxParams cp;
  cp.N = p.N;
  cp.L = p.L;
  cp.q.assign(p.q, p.q + p.L);
  cp.psi.assign(p.psi, p.psi + p.L);
  cp.plaintext_modulus = p.scale_bits;
  cp.batch = p.batch;
  cp.sigma = (float)p.sigma;
  // the block ends (..., ks = HYBRID 2, rs = EXACTRESCALE 1, dnum): dnum follows multDepth
  // (2 for the reference's multDepth 1 and for key-eval-mult.txt's multDepth 2; special_primes)
  uint32_t dn, al, kp;
  uint64_t sp[kMaxTowers];
  special_primes(p.N, p.L, p.q, &dn, &al, &kp, sp, nullptr);
  cp.fields.back() = dn;
  return cp;
}

// PALISADE's GenerateUniqueKeyID: four 32-bit draws, 8 lowercase hex digits each
static std::string make_keytag(const shelfi_ctx* ctx) {
  uint32_t r[4];
  if (ctx->seed) {
    uint32_t k[8];
    seed_to_key(ctx->seed ^ 0x6b65797461670000ull, k);  // "keytag"
    std::memcpy(r, k, sizeof(r));
  } else {
    os_random(r, sizeof(r));
  }
  char buf[33];
  for (int i = 0; i < 4; ++i) std::snprintf(buf + 8 * i, 9, "%08x", r[i]);
  return std::string(buf, 32);
}

}  // namespace shelfi

// ============================================================== C ABI ======
extern "C" {

int shelfi_abi_version(void) { return SHELFI_ABI_VERSION; }
const char* shelfi_last_error(void) { return g_last_error.c_str(); }
void shelfi_free(void* p) { std::free(p); }

int shelfi_params_generate(uint32_t ring_dim, uint32_t num_towers, uint32_t scale_bits,
                           uint32_t first_mod_bits, uint32_t batch, uint32_t* ring_dim_out,
                           uint64_t* moduli_out, uint64_t* roots_out) {
  return guarded([&] {
    uint32_t N = ring_dim ? ring_dim
                          : default_ring_dim(num_towers, scale_bits, first_mod_bits, batch);
    if (!N) throw Error{SHELFI_ERR_ARG, "no ring dimension satisfies the security/batch constraints"};
    validate_params(N, num_towers, scale_bits, first_mod_bits, batch);
    uint64_t q[kMaxTowers], psi[kMaxTowers];
    generate_chain(N, num_towers, scale_bits, first_mod_bits, q, psi);
    if (ring_dim_out) *ring_dim_out = N;
    for (uint32_t t = 0; t < num_towers; ++t) {
      if (moduli_out) moduli_out[t] = q[t];
      if (roots_out) roots_out[t] = psi[t];
    }
  });
}

int shelfi_read_palisade(const char* cryptodir, uint32_t* ring_dim, uint32_t* num_towers,
                         uint64_t* moduli, uint64_t* roots, uint64_t* pk, uint64_t* sk) {
  if (!cryptodir) return SHELFI_ERR_ARG;
  return guarded([&] {
    const std::string dir(cryptodir);
    PalisadeContext pc = palisade_read_context(read_file(dir + "cryptocontext.txt"));
    const uint32_t L = (uint32_t)pc.q.size();
    if (ring_dim) *ring_dim = pc.N;
    if (num_towers) *num_towers = L;
    for (uint32_t t = 0; t < L; ++t) {
      if (moduli) moduli[t] = pc.q[t];
      if (roots) roots[t] = pc.psi[t];
    }
    if (pk || sk) {
      std::vector<uint64_t> p, s;
      palisade_read_keys(read_file(dir + "key-public.txt"), read_file(dir + "key-private.txt"),
                         pc.N, pc.q, p, s);
      if (pk) std::memcpy(pk, p.data(), p.size() * 8);
      if (sk) std::memcpy(sk, s.data(), s.size() * 8);
    }
  });
}

int shelfi_ctx_create(uint32_t ring_dim, uint32_t num_towers, uint32_t scale_bits,
                      uint32_t first_mod_bits, uint32_t batch, int device, shelfi_ctx** out) {
  if (!out) return SHELFI_ERR_ARG;
  *out = nullptr;
  shelfi_ctx* ctx = new (std::nothrow) shelfi_ctx();
  if (!ctx) return SHELFI_ERR_DEVICE;
  reload_switches();  // the process-wide probe switches are re-read when a context is created
  int rc = guarded([&] {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
      throw Error{SHELFI_ERR_DEVICE, "no HIP device available (libshelfi requires an MI355X / gfx950)"};
    if (device < 0 || device >= count) throw Error{SHELFI_ERR_ARG, "device ordinal out of range"};
    hipDeviceProp_t prop;
    SHELFI_HIP(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
      throw Error{SHELFI_ERR_DEVICE, std::string("device is ") + prop.gcnArchName +
                                         "; libshelfi is built for gfx950 only"};
    ctx->device = device;
    DeviceGuard g(device);
    uint32_t N = ring_dim ? ring_dim
                          : default_ring_dim(num_towers, scale_bits, first_mod_bits, batch);
    if (!N) throw Error{SHELFI_ERR_ARG, "no ring dimension satisfies the security/batch constraints"};
    validate_params(N, num_towers, scale_bits, first_mod_bits, batch);
    uint64_t q[kMaxTowers], psi[kMaxTowers];
    generate_chain(N, num_towers, scale_bits, first_mod_bits, q, psi);
    SHELFI_HIP(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    SHELFI_HIP(hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking));
    SHELFI_HIP(hipStreamCreateWithFlags(&ctx->stream3, hipStreamNonBlocking));
    SHELFI_HIP(hipMalloc(&ctx->dev_flag, 32));
    SHELFI_HIP(hipHostMalloc((void**)&ctx->host_flag, 32, hipHostMallocDefault));
    // GenFlag words: pinned, mapped and coherent host memory the kernels store to (system scope)
    SHELFI_HIP(hipHostMalloc((void**)&ctx->map_flag_host, 64, hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(ctx->map_flag_host, 0, 64);
    SHELFI_HIP(hipHostGetDevicePointer((void**)&ctx->map_flag_dev, ctx->map_flag_host, 0));
    set_params(ctx, N, num_towers, scale_bits, first_mod_bits, batch, q, psi);
  });
  if (rc != SHELFI_OK) {
    shelfi_ctx_destroy(ctx);
    return rc;
  }
  *out = ctx;
  return SHELFI_OK;
}

void shelfi_ctx_destroy(shelfi_ctx* ctx) {
  if (!ctx) return;
  {
    int prev = -1;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);
    if (ctx->stream3) (void)hipStreamSynchronize(ctx->stream3);
    comm_release(ctx);
    free_keys(ctx);
    free_tables(ctx);
    delete ctx->stage;
    ctx->stage = nullptr;
    delete ctx->drain;
    ctx->drain = nullptr;
    delete ctx->up2;
    ctx->up2 = nullptr;
    if (ctx->stream4) (void)hipStreamDestroy(ctx->stream4);
    ctx->stream4 = nullptr;
    for (int i = 0; i < shelfi_ctx::kWeightRing; ++i) {
      if (ctx->wl_done[i]) (void)hipEventSynchronize(ctx->wl_done[i]);
      if (ctx->wl_done[i]) (void)hipEventDestroy(ctx->wl_done[i]);
      if (ctx->wl_dev[i]) (void)hipFree(ctx->wl_dev[i]);
    }
    dfree_t(ctx->unit_wl);
    if (ctx->poly_pin) (void)hipHostFree(ctx->poly_pin);
    ctx->poly_pin = nullptr;
    dfree_t(ctx->scratch);
    dfree_t(ctx->io);
    if (ctx->gather_host) (void)hipHostFree(ctx->gather_host);
    ctx->gather_host = nullptr;
    dfree_t(ctx->dev_flag);
    if (ctx->host_flag) (void)hipHostFree(ctx->host_flag);
    ctx->host_flag = nullptr;
    if (ctx->map_flag_host) (void)hipHostFree(ctx->map_flag_host);
    ctx->map_flag_host = ctx->map_flag_dev = nullptr;
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
    if (ctx->stream3) (void)hipStreamDestroy(ctx->stream3);
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  delete ctx;
}

int shelfi_ctx_info(const shelfi_ctx* ctx, shelfi_info* o) {
  if (!ctx || !o) return SHELFI_ERR_ARG;
  std::memset(o, 0, sizeof(*o));
  o->ring_dim = ctx->p.N;
  o->num_towers = ctx->p.L;
  o->batch = ctx->p.batch;
  o->scale_bits = ctx->p.scale_bits;
  o->first_mod_bits = ctx->p.first_mod_bits;
  o->device = ctx->device;
  for (uint32_t t = 0; t < ctx->p.L; ++t) {
    o->moduli[t] = ctx->p.q[t];
    o->roots[t] = ctx->p.psi[t];
  }
  o->delta = ctx->p.delta;
  o->key_id = ctx->key_id;
  o->keys_loaded = ctx->keys_loaded ? 1 : 0;
  o->palisade_keys = ctx->palisade_keys ? 1 : 0;
  o->slot_packing = ctx->p.pack;
  o->values_per_ct = (uint32_t)values_per_ct(ctx->p);
  return SHELFI_OK;
}

int shelfi_set_seed(shelfi_ctx* ctx, uint64_t seed) {
  if (!ctx) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->seed = seed;
  ctx->enc_counter = 0;
  ctx->thr_counter = 0;
  return SHELFI_OK;
}

int shelfi_set_keys(shelfi_ctx* ctx, const uint64_t* pk, const uint64_t* sk) {
  if (!ctx || !pk || !sk) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    DeviceGuard g(ctx->device);
    install_keys(ctx, pk, sk, false);
  });
}

int shelfi_get_keys(const shelfi_ctx* ctx, uint64_t* pk, uint64_t* sk) {
  if (!ctx) return SHELFI_ERR_ARG;
  if (!ctx->keys_loaded) {
    set_error("no keys loaded");
    return SHELFI_ERR_STATE;
  }
  if (pk) std::memcpy(pk, ctx->pk_host.data(), ctx->pk_host.size() * sizeof(uint64_t));
  if (sk) std::memcpy(sk, ctx->sk_host.data(), ctx->sk_host.size() * sizeof(uint64_t));
  return SHELFI_OK;
}

int shelfi_keygen(shelfi_ctx* ctx, const char* cryptodir) {
  if (!ctx) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    DeviceGuard g(ctx->device);
    const Params& p = ctx->p;
    const size_t LN = (size_t)p.L * p.N;
    std::vector<uint64_t> sk(LN), pk(2 * LN);
    {
      uint32_t key[8];
      KeyWiper wipe(key);
      stream_key(ctx, key);
      DevWords sk_d(LN), pk_d(2 * LN);
      void* scratch = ensure(ctx->scratch, ctx->scratch_bytes, keygen_scratch_bytes(p));
      launch_keygen(p, ctx->dt, key, sk_d.p, pk_d.p, scratch, ctx->stream);
      SHELFI_HIP(hipMemcpyAsync(sk.data(), sk_d.p, LN * 8, hipMemcpyDeviceToHost, ctx->stream));
      SHELFI_HIP(hipMemcpyAsync(pk.data(), pk_d.p, 2 * LN * 8, hipMemcpyDeviceToHost, ctx->stream));
      SHELFI_HIP(hipStreamSynchronize(ctx->stream));
    }
    install_keys(ctx, pk.data(), sk.data(), true);
    // ckks.cpp:36-56: context first, then public, then private key, in PALISADE 1.11's
    // cereal PortableBinary format (palisade_codec.h), so PALISADE clients can load them
    const PalisadeCtxParams cp = palisade_params_of(ctx->p);
    std::string tag = make_keytag(ctx);
    if (cryptodir && *cryptodir) {
      const std::string dir(cryptodir);
      write_file(dir + "cryptocontext.txt", palisade_context_file(cp));
      write_file(dir + "key-public.txt", palisade_key_file(cp, tag, pk.data(), true));
      write_file(dir + "key-private.txt", palisade_key_file(cp, tag, sk.data(), false));
    }
    ctx->pal_ctx_obj = palisade_context_object(cp, 3);
    ctx->pal_keytag = std::move(tag);
  });
}

int shelfi_multiparty_keygen(shelfi_ctx* ctx, const uint64_t* prev_pk) {
  if (!ctx || !prev_pk) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    DeviceGuard g(ctx->device);
    const Params& p = ctx->p;
    const size_t LN = (size_t)p.L * p.N;
    for (size_t i = 0; i < 2 * LN; ++i)
      if (prev_pk[i] >= p.q[(i / p.N) % p.L]) throw Error{SHELFI_ERR_FORMAT, "previous public key residue >= q"};
    uint32_t key[8];
    KeyWiper wipe(key);
    stream_key(ctx, key);
    DevWords sk_d(LN), pk_d(2 * LN), prev_d(2 * LN);
    void* scratch = ensure(ctx->scratch, ctx->scratch_bytes, keygen_chain_scratch_bytes(p));
    std::vector<uint64_t> sk(LN), pk(2 * LN);
    SHELFI_HIP(hipMemcpyAsync(prev_d.p, prev_pk, 2 * LN * 8, hipMemcpyHostToDevice, ctx->stream));
    launch_keygen_chain(p, ctx->dt, key, prev_d.p, sk_d.p, pk_d.p, scratch, ctx->stream);
    SHELFI_HIP(hipMemcpyAsync(sk.data(), sk_d.p, LN * 8, hipMemcpyDeviceToHost, ctx->stream));
    SHELFI_HIP(hipMemcpyAsync(pk.data(), pk_d.p, 2 * LN * 8, hipMemcpyDeviceToHost, ctx->stream));
    SHELFI_HIP(hipStreamSynchronize(ctx->stream));
    install_keys(ctx, pk.data(), sk.data(), false);
    ctx->threshold_share = true;
  });
}

int shelfi_set_threshold_noise(shelfi_ctx* ctx, double sigma) {
  if (!ctx || !std::isfinite(sigma) || sigma < 0.0 || sigma > 0x1.0p40) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  ctx->thr_sigma = sigma;
  return SHELFI_OK;
}

int shelfi_load(shelfi_ctx* ctx, const char* cryptodir) {
  if (!ctx || !cryptodir) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    DeviceGuard g(ctx->device);
    const std::string dir(cryptodir);
    const std::string cc = read_file(dir + "cryptocontext.txt");
    if (cc.size() >= 4 && cc.compare(0, 4, "SHCC") == 0) {
      size_t off = 4;
      if (get<uint32_t>(cc, off) != 1) throw Error{SHELFI_ERR_FORMAT, "unsupported context version"};
      const uint32_t N = get<uint32_t>(cc, off), L = get<uint32_t>(cc, off);
      const uint32_t batch = get<uint32_t>(cc, off), sb = get<uint32_t>(cc, off);
      const uint32_t fb = get<uint32_t>(cc, off);
      const double sigma = get<double>(cc, off);
      if (L < 1 || L > (uint32_t)kMaxTowers) throw Error{SHELFI_ERR_FORMAT, "bad tower count"};
      uint64_t q[kMaxTowers], psi[kMaxTowers];
      for (uint32_t t = 0; t < L; ++t) q[t] = get<uint64_t>(cc, off);
      for (uint32_t t = 0; t < L; ++t) psi[t] = get<uint64_t>(cc, off);
      validate_params(N, L, sb, fb, batch);
      free_keys(ctx);
      set_params(ctx, N, L, sb, fb, batch, q, psi);
      ctx->p.sigma = sigma;
      const size_t LN = (size_t)L * N;
      const std::string ps = read_file(dir + "key-public.txt");
      const std::string ss = read_file(dir + "key-private.txt");
      size_t po = 4, so = 4;
      if (ps.compare(0, 4, "SHPK") != 0 || ss.compare(0, 4, "SHSK") != 0)
        throw Error{SHELFI_ERR_FORMAT, "key files do not match the context format"};
      (void)get<uint32_t>(ps, po);
      (void)get<uint32_t>(ss, so);
      if (get<uint64_t>(ps, po) != ctx->params_id || get<uint64_t>(ss, so) != ctx->params_id)
        throw Error{SHELFI_ERR_FORMAT, "key files were generated for a different context"};
      if (ps.size() != po + 2 * LN * 8 || ss.size() != so + LN * 8)
        throw Error{SHELFI_ERR_FORMAT, "key file size mismatch"};
      install_keys(ctx, reinterpret_cast<const uint64_t*>(ps.data() + po),
                   reinterpret_cast<const uint64_t*>(ss.data() + so), false);
    } else {
      // PALISADE 1.11 cereal-binary files (the reference's committed key material)
      PalisadeContext pc = palisade_read_context(cc);
      const uint32_t N = pc.N, L = (uint32_t)pc.q.size();
      const uint32_t batch = std::min<uint32_t>(ctx->p.batch, N / 2);
      // the scaling-factor bits the context was generated with (its plaintext-modulus
      // field), when the file has the layout palisade_codec.h restates
      uint32_t sb = ctx->p.scale_bits;
      try {
        const PalisadeCtxParams cp = palisade_parse_context_file(cc);
        if (cp.plaintext_modulus >= 10 && cp.plaintext_modulus <= 58) sb = (uint32_t)cp.plaintext_modulus;
      } catch (const Error&) {
      }
      const uint32_t fb = std::max(ctx->p.first_mod_bits, sb);
      validate_params(N, L, sb, fb, batch);
      free_keys(ctx);
      set_params(ctx, N, L, sb, fb, batch, pc.q.data(), pc.psi.data());
      std::vector<uint64_t> pk, sk;
      const std::string pub = read_file(dir + "key-public.txt");
      palisade_read_keys(pub, read_file(dir + "key-private.txt"), N, pc.q, pk, sk);
      std::string ctx_obj, keytag;
      palisade_key_context(pub, ctx_obj, keytag);  // for PALISADE-format output (§8 f1)
      install_keys(ctx, pk.data(), sk.data(), true);
      ctx->pal_ctx_obj = std::move(ctx_obj);
      ctx->pal_keytag = std::move(keytag);
      load_evalkey_if_present(ctx, dir);  // §8 f4: a key-eval-mult.txt of these keys
    }
  });
}

int shelfi_fft_twiddles(uint32_t slots, double* ir, double* ii, double* fr, double* fi) {
  if (!slots || (slots & (slots - 1)) || !ir || !ii || !fr || !fi) return SHELFI_ERR_ARG;
  fft_twiddles(slots, ir, ii, fr, fi);
  return SHELFI_OK;
}

int shelfi_gauss_cdt(double sigma, uint64_t* cdt, int max_entries) {
  if (!cdt) return SHELFI_ERR_ARG;
  return gauss_cdt(sigma, cdt, max_entries);
}

}  // extern "C"
