// seeded.hip — seeded ciphertexts: a learner that holds the secret key encrypts
// symmetrically, c1 = a uniform and c0 = NTT(m + e) - a . NTT(s), and a is expanded from a 32-byte public
// seed on whichever side needs it, so only c0 travels.
//
// Kernels:
//   seeded_sample_kernel   encode's rounding + encrypt's e0 of the same key and index, m + e0 reduced into
//                          every tower (canonical, COEFFICIENT); the generic forward NTT follows
//   seeded_c0_kernel       c0 = NTT(m + e0) - a . NTT(s) in place, a drawn in registers and never stored
//   seeded_expand_kernel   polynomial 1 of ciphertexts [k0, k0 + kn) of a [kn][2][Lu][N] batch
// The c1 stream (nonce domain 9): for ciphertext k of its blob, tower t and coefficient j of the stored
// EVALUATION order, the ChaCha20 block of the seed with counter j >> 2 and nonce (9 << 56) | (k << 8) | t,
// read as eight 64-bit words; lo = word 2 (j & 3), hi = the next, a = (hi 2^64 + lo) mod q_t -- keygen's
// draw of a_t exactly.  a is uniform in the EVALUATION domain: no transform.
#include <hip/hip_runtime.h>

#include "dev_common.h"
#include "shelfi_internal.h"
#include "transform_dev.h"

namespace shelfi {

constexpr uint64_t kSeededDomain = 9ull << 56;

// a[u] = the stream's residue j0 + u of row (k, t), j0 a multiple of 8: two blocks
__device__ __forceinline__ void seeded_draw8(const Key8& seed, uint64_t k, uint32_t t, uint32_t j0,
                                             const TowerConst& c, uint64_t (&a)[8]) {
  const uint64_t nonce = kSeededDomain | (k << 8) | t;
  uint64_t ra[16];
  chacha20_block(seed, j0 >> 2, nonce, ra);
  chacha20_block(seed, (j0 >> 2) + 1, nonce, ra + 8);
#pragma unroll
  for (int u = 0; u < 8; ++u)
    a[u] = addmod(shoup_mul(red64(ra[2 * u + 1], c.q, c.one_shoup), c.r64, c.r64_shoup, c.q),
                  red64(ra[2 * u], c.q, c.one_shoup), c.q);
}

// The mapping of seeded_c0_kernel and seeded_expand_kernel (keygen's arrangement): one thread = 8
// consecutive residues of one (k, t) row, the row block-uniform so the tower's constants sit in SGPRs;
// bpr blocks a row.  Returns false for the threads past a ring of fewer than 2048 coefficients.
__device__ __forceinline__ bool seeded_row(uint32_t logN, uint32_t bpr, uint64_t& row, uint32_t& j0) {
  row = blockIdx.x / bpr;
  const uint32_t gid = (blockIdx.x % bpr) * 256 + threadIdx.x;
  j0 = gid * 8;
  return gid < ((1u << logN) >> 3);
}

__global__ __launch_bounds__(256) void seeded_expand_kernel(Key8 seed, uint64_t k0, uint32_t Lu, uint32_t logN,
                                                            uint32_t bpr, const TowerConst* __restrict__ tcs,
                                                            uint64_t* __restrict__ ct) {
  uint64_t row;
  uint32_t j0;
  if (!seeded_row(logN, bpr, row, j0)) return;
  const uint64_t k = row / Lu;
  const uint32_t t = (uint32_t)(row - k * Lu);
  const TowerConst& c = tcs[t];
  uint64_t a[8];
  seeded_draw8(seed, k0 + k, t, j0, c, a);
  ulonglong2* o = reinterpret_cast<ulonglong2*>(ct + (((k * 2 + 1) * Lu + t) << logN) + j0);
#pragma unroll
  for (int u = 0; u < 4; ++u) o[u] = make_ulonglong2(a[2 * u], a[2 * u + 1]);
}

// x [kn][L][N] holds NTT(m + e0), canonical; sk, sk_sh the secret key and its Shoup companions
__global__ __launch_bounds__(256) void seeded_c0_kernel(Key8 seed, uint64_t k0, uint32_t L, uint32_t logN,
                                                        uint32_t bpr, const TowerConst* __restrict__ tcs,
                                                        const uint64_t* __restrict__ sk,
                                                        const uint64_t* __restrict__ sk_sh, uint64_t* x) {
  uint64_t row;
  uint32_t j0;
  if (!seeded_row(logN, bpr, row, j0)) return;
  const uint64_t k = row / L;
  const uint32_t t = (uint32_t)(row - k * L);
  const TowerConst& c = tcs[t];
  uint64_t a[8];
  seeded_draw8(seed, k0 + k, t, j0, c, a);
  const ulonglong2* s = reinterpret_cast<const ulonglong2*>(sk + ((uint64_t)t << logN) + j0);
  const ulonglong2* sp = reinterpret_cast<const ulonglong2*>(sk_sh + ((uint64_t)t << logN) + j0);
  ulonglong2* o = reinterpret_cast<ulonglong2*>(x + (row << logN) + j0);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const ulonglong2 w = s[u], wp = sp[u], v = o[u];
    o[u] = make_ulonglong2(submod(v.x, shoup_mul(a[2 * u], w.x, wp.x, c.q), c.q),
                           submod(v.y, shoup_mul(a[2 * u + 1], w.y, wp.y, c.q), c.q));
  }
}

// One thread = sample group h of ciphertext k, the 16 coefficients j = h + (N/16) i (enc_prep_kernel's
// mapping, rounding and e0 stream, without v and e1): m + e0 into every tower of out [K][L][N].
__global__ __launch_bounds__(256) void seeded_sample_kernel(const double2* __restrict__ fbuf, uint64_t K,
                                                            uint32_t logN, uint32_t logS, uint32_t L, double delta,
                                                            const uint64_t* __restrict__ cdt, int T, Key8 key,
                                                            uint64_t g0, const TowerConst* __restrict__ tcs,
                                                            uint64_t* __restrict__ out, GenFlag flag) {
  const uint32_t N = 1u << logN, S = 1u << logS, N16 = N >> 4, V0 = N >> 6;
  __shared__ uint32_t thi[64], tlo[64];
  load_cdt32(cdt, T, thi, tlo);
  __syncthreads();
  const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t k = gid >> (logN - 4);
  if (k >= K) return;
  const uint32_t h = (uint32_t)(gid & (N16 - 1));
  const uint64_t nonce = (1ull << 56) | (g0 + k);
  const uint32_t half = N >> 1, gapLog = logN - 1 - logS;
  const double dS = (double)S;
  const double lim = 2305843009213693952.0;  // 2^61: beyond, the call is refused
  uint32_t w[16];
  chacha20_block32(key, V0 + h, nonce, w);
  int64_t me[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint32_t j = h + N16 * i;
    const uint32_t jj = j < half ? j : j - half;
    int64_t m = 0;
    if ((jj & ((1u << gapLog) - 1)) == 0) {
      const double2 cv = fbuf[k * S + bitrev_dev(jj >> gapLog, logS)];
      const double val = __dmul_rn(__ddiv_rn(j < half ? cv.x : cv.y, dS), delta);
      if (!(fabs(val) <= lim)) {
        gen_flag_set(flag, 0);
        if (!isfinite(val)) gen_flag_set(flag, 1);
      }
      m = round_half_away(val);
    }
    me[i] = m + gauss32(w[i], thi, tlo, [&] { return chacha20_word(key, V0 + 2 * N16 + h, nonce, i); });
  }
#pragma unroll 1
  for (uint32_t t = 0; t < L; ++t) {
    const TowerConst c = tcs[t];
    uint64_t* __restrict__ o = out + ((k * L + t) << logN) + h;
#pragma unroll
    for (int i = 0; i < 16; ++i) o[(uint64_t)N16 * i] = mod_signed_dev(me[i], c);
  }
}

static Key8 key8_of(const uint32_t w[8]) {
  Key8 k;
  for (int i = 0; i < 8; ++i) k.k[i] = w[i];
  return k;
}

// blocks of the 8-residues-a-thread kernels over `rows` (k, t) rows
static uint32_t seeded_grid(uint64_t rows, uint32_t logN, uint32_t* bpr) {
  *bpr = logN > 11 ? 1u << (logN - 11) : 1;
  const uint64_t blocks = rows * *bpr;
  if (blocks > 0x7FFFFFFFull) throw Error{SHELFI_ERR_ARG, "seeded batch too large"};
  return (uint32_t)blocks;
}

void launch_seeded_expand(const uint32_t seed[8], uint64_t k0, uint64_t kn, uint32_t Lu, uint32_t logN,
                          const TowerConst* tc, uint64_t* ct, hipStream_t s) {
  if (!kn) return;
  if (k0 + kn > kSeededMaxCts) throw Error{SHELFI_ERR_ARG, "seeded batch: ciphertext index at or above 2^48"};
  uint32_t bpr;
  const uint32_t blocks = seeded_grid(kn * Lu, logN, &bpr);
  hipLaunchKernelGGL(seeded_expand_kernel, dim3(blocks), dim3(256), 0, s, key8_of(seed), k0, Lu, logN, bpr, tc, ct);
  SHELFI_HIP(hipGetLastError());
}

size_t seeded_encrypt_scratch_bytes(const Params& p, uint64_t K) { return encode_scratch_bytes(p, K); }

void launch_encrypt_seeded(const Params& p, const DeviceTables& dt, const DeviceKeys& dk, const double* x, uint64_t n,
                           uint64_t K, uint64_t* c0, void* scratch, const uint32_t key[8], uint64_t g0,
                           const uint32_t seed[8], uint64_t k0, GenFlag flag, hipStream_t s) {
  if (!K) return;
  if (k0 + K > kSeededMaxCts) throw Error{SHELFI_ERR_ARG, "seeded batch: ciphertext index at or above 2^48"};
  const uint32_t logS = __builtin_ctz(p.batch);
  double2* fbuf = reinterpret_cast<double2*>(scratch);
  launch_encode_fft(p, dt, x, n, K, fbuf, s);
  const uint64_t threads = K << (p.logN - 4);
  if ((threads + 255) / 256 > 0x7FFFFFFFull) throw Error{SHELFI_ERR_ARG, "seeded batch too large"};
  hipLaunchKernelGGL(seeded_sample_kernel, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, s, fbuf, K, p.logN,
                     logS, p.L, p.delta, dt.cdt, dt.cdt_len, key8_of(key), g0, dt.tc, c0, flag);
  SHELFI_HIP(hipGetLastError());
  launch_ntt(c0, K * p.L, p.L, p.logN, false, dt, s);
  uint32_t bpr;
  const uint32_t blocks = seeded_grid(K * p.L, p.logN, &bpr);
  hipLaunchKernelGGL(seeded_c0_kernel, dim3(blocks), dim3(256), 0, s, key8_of(seed), k0, p.L, p.logN, bpr, dt.tc,
                     dk.sk, dk.sk_sh, c0);
  SHELFI_HIP(hipGetLastError());
}

}  // namespace shelfi
