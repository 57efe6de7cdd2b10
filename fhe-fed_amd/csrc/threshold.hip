// threshold.hip — partial decryption of the threshold scheme (mkhe.cpp:395-400: each party's
// MultipartyDecryptLead / MultipartyDecryptMain of the aggregate).
//
//   out[k][t] = [c0 +] c1 * sk_i + NTT(e_k),  e_k = round(sigma z), one integer polynomial per ciphertext
//
// sigma = 0 (parity mode): pd_plain_kernel, one element-wise pass (reads 1 or 2 polynomials and the
// key's {s, s'}, writes 1; HBM-bound).
// sigma > 0: the noise takes the forward NTT's two passes, as encrypt's error polynomials do:
//   pd_noise_cols    samples the integers on load (ChaCha20 + box_muller), reduces them into each tower
//                    and runs the first logN - BL stages on register columns -> scratch [K][towers][N], lazy
//   pd_blocks_ct     the block stages at compile-time shape (fwd_block_pass_ct); [c0 +] c1 * s + E is formed
//                    in the last chunk's store epilogue, straight from registers
//   pd_blocks        the generic LDS block pass with the same epilogue: rings of one block (N <= 2^11,
//                    sampled on load, no columns pass and no scratch) and towers below 2^40
// so NTT(e) never exists in HBM.
//
// Noise stream of ciphertext k: ChaCha20 under the call's key, nonce (5 << 56) | (g0 + k).  A block's 8
// 64-bit words give 16 normals (word u -> normals 2u, 2u + 1: box_muller of its low and high halves).
// With R = 2^(logN - BL) rows (coefficient j = row * 2^BL + col): R = 1: block j >> 4, normal j & 15;
// R > 1: column col owns blocks col * nb .. col * nb + nb - 1 (nb = max(1, R / 16)), row r takes normal
// r of them (a column of fewer than 16 rows leaves the rest of its block unused).
#include <hip/hip_runtime.h>

#include "dev_common.h"
#include "shelfi_internal.h"

namespace shelfi {

struct PdNoise {
  Key8 key;
  uint64_t g0;
  double sigma;
};
constexpr uint64_t kPdNonce = 5ull << 56;

// the 16 integers of one stream block
__device__ __forceinline__ void pd_block16(const PdNoise& nz, uint64_t k, uint64_t blk, int64_t (&e)[16]) {
  uint64_t w[8];
  chacha20_block(nz.key, blk, kPdNonce | (nz.g0 + k), w);
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    double z0, z1;
    box_muller((uint32_t)w[u], (uint32_t)(w[u] >> 32), z0, z1);
    e[2 * u] = round_half_away(nz.sigma * z0);
    e[2 * u + 1] = round_half_away(nz.sigma * z1);
  }
}

// [c0 +] c1 * s + E for the 16-byte pair at element `e` of [towers][N] of ciphertext k
__device__ __forceinline__ void pd_store_pair(const uint64_t* __restrict__ ct, const uint64_t* __restrict__ sk,
                                              const uint64_t* __restrict__ sksh, uint64_t* __restrict__ out,
                                              uint64_t k, uint64_t TN, uint64_t e, uint64_t q, bool lead,
                                              ulonglong2 E) {
  const ulonglong2 c1 = *reinterpret_cast<const ulonglong2*>(ct + (2 * k + 1) * TN + e);
  const ulonglong2 s = *reinterpret_cast<const ulonglong2*>(sk + e);
  const ulonglong2 ss = *reinterpret_cast<const ulonglong2*>(sksh + e);
  ulonglong2 v = make_ulonglong2(addmod(shoup_mul(c1.x, s.x, ss.x, q), E.x, q),
                                 addmod(shoup_mul(c1.y, s.y, ss.y, q), E.y, q));
  if (lead) {
    const ulonglong2 c0 = *reinterpret_cast<const ulonglong2*>(ct + 2 * k * TN + e);
    v = make_ulonglong2(addmod(v.x, c0.x, q), addmod(v.y, c0.y, q));
  }
  *reinterpret_cast<ulonglong2*>(out + k * TN + e) = v;
}

// sigma = 0: one thread per 16-byte pair of out [K][towers][N]
__global__ __launch_bounds__(256) void pd_plain_kernel(const uint64_t* __restrict__ ct,
                                                       const uint64_t* __restrict__ sk,
                                                       const uint64_t* __restrict__ sksh,
                                                       const TowerConst* __restrict__ tcs, uint32_t towers,
                                                       uint32_t logN, uint64_t pairs, int lead,
                                                       uint64_t* __restrict__ out) {
  const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= pairs) return;
  const uint64_t TN = (uint64_t)towers << logN;
  const uint64_t k = (2 * p) / TN, e = 2 * p - k * TN;
  const uint64_t q = tcs[e >> logN].q;
  pd_store_pair(ct, sk, sksh, out, k, TN, e, q, lead != 0, make_ulonglong2(0, 0));
}

// The noise's columns pass: thread = column `col` of ciphertext k, its R rows sampled once and taken
// through every tower (ntt_fwd_cols' stages; lazy values below 8q to ebuf [K][towers][N]).
template <int LOGR>
__global__ __launch_bounds__(256) void pd_noise_cols(uint64_t* __restrict__ ebuf, uint32_t towers, uint32_t logN,
                                                     const uint64_t* __restrict__ tw,
                                                     const uint64_t* __restrict__ twp,
                                                     const TowerConst* __restrict__ tcs, PdNoise nz) {
  constexpr int R = 1 << LOGR, NB = R >= 16 ? R / 16 : 1;
  const uint32_t N = 1u << logN;
  const uint32_t BLK = N >> LOGR;
  const uint32_t bpp = BLK / 256;
  const uint64_t k = blockIdx.x / bpp;
  const uint32_t col = (blockIdx.x % bpp) * 256 + threadIdx.x;
  int64_t ev[R];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    int64_t e16[16];
    pd_block16(nz, k, (uint64_t)col * NB + i, e16);
#pragma unroll
    for (int u = 0; u < 16; ++u)
      if (16 * i + u < R) ev[16 * i + u] = e16[u];
  }
  for (uint32_t t = 0; t < towers; ++t) {
    const TowerConst& c = tcs[t];
    const uint64_t q = c.q;
    const uint64_t* __restrict__ w = tw + (uint64_t)t * N;
    const uint64_t* __restrict__ wp = twp + (uint64_t)t * N;
    uint64_t x[R];
#pragma unroll
    for (int r = 0; r < R; ++r) x[r] = mod_signed_dev(ev[r], c);
#pragma unroll
    for (int s = 0; s < LOGR; ++s) {
      const int m = 1 << s, tr = R >> (s + 1);
#pragma unroll
      for (int i = 0; i < m; ++i) {
        const uint64_t W = w[m + i], Wp = wp[m + i];
#pragma unroll
        for (int jj = 0; jj < tr; ++jj) {
          const int r0 = 2 * i * tr + jj, r1 = r0 + tr;
          ct_bfly(x[r0], x[r1], W, Wp, q);
        }
      }
    }
    uint64_t* __restrict__ a = ebuf + ((k * towers + t) << logN) + col;
#pragma unroll
    for (int r = 0; r < R; ++r) a[(uint64_t)r * BLK] = x[r];
  }
}

// The noise's block stages at compile-time shape + the combine in the last chunk's epilogue.
template <int BL, int K1, int K2, int K3, int K4>
__global__ __launch_bounds__(256) void pd_blocks_ct(const uint64_t* __restrict__ ebuf, uint32_t towers,
                                                    uint32_t logN, const ulonglong2* __restrict__ twb,
                                                    const TowerConst* __restrict__ tcs,
                                                    const uint64_t* __restrict__ ct,
                                                    const uint64_t* __restrict__ sk,
                                                    const uint64_t* __restrict__ sksh, int lead,
                                                    uint64_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint64_t sm[lpad_size(BL)];
  const uint32_t sh = logN - BL;
  const uint64_t poly = blockIdx.x >> sh;  // k * towers + t
  const uint32_t b = blockIdx.x & ((1u << sh) - 1);
  const uint32_t t = (uint32_t)(poly % towers);
  const uint64_t k = poly / towers;
  const TowerConst& c = tcs[t];
  const uint64_t TN = (uint64_t)towers << logN;
  const uint64_t off = ((uint64_t)t << logN) + ((uint64_t)b << BL);
  fwd_block_pass_ct<BL, K1, K2, K3, K4>(ebuf + (poly << logN) + ((uint64_t)b << BL), twb + off, c.q, c.n8q, sm,
                                        [&](uint32_t j0, auto& x) {
#pragma unroll
                                          for (int m = 0; m < (1 << K4); m += 2)
                                            pd_store_pair(ct, sk, sksh, out, k, TN, off + j0 + m, c.q, lead != 0,
                                                          make_ulonglong2(red_any(x[m], c), red_any(x[m + 1], c)));
                                        });
}

// The generic block pass (ntt_fwd_blocks' stages in LDS) with the same epilogue.  sstart = 0: the ring
// is one block and the integers are sampled while LDS is filled (ebuf unused).
__global__ __launch_bounds__(256) void pd_blocks(const uint64_t* __restrict__ ebuf, uint32_t towers, uint32_t logN,
                                                 uint32_t sstart, const uint64_t* __restrict__ tw,
                                                 const uint64_t* __restrict__ twp,
                                                 const TowerConst* __restrict__ tcs,
                                                 const uint64_t* __restrict__ ct,
                                                 const uint64_t* __restrict__ sk,
                                                 const uint64_t* __restrict__ sksh, int lead,
                                                 uint64_t* __restrict__ out, PdNoise nz) {
  extern __shared__ __attribute__((aligned(16))) uint64_t sm[];
  const uint32_t blkLog = logN - sstart, blk = 1u << blkLog;
  const uint64_t poly = blockIdx.x >> sstart;
  const uint32_t b = blockIdx.x & ((1u << sstart) - 1);
  const uint32_t t = (uint32_t)(poly % towers);
  const uint64_t k = poly / towers;
  const TowerConst& c = tcs[t];
  const uint64_t q = c.q;
  if (sstart == 0) {
    for (uint32_t i = threadIdx.x; i < blk / 16; i += 256) {
      int64_t e16[16];
      pd_block16(nz, k, i, e16);
#pragma unroll
      for (int u = 0; u < 16; ++u) sm[lds_sw(16 * i + u)] = mod_signed_dev(e16[u], c);
    }
  } else {
    const ulonglong2* src = reinterpret_cast<const ulonglong2*>(ebuf + (poly << logN) + ((uint64_t)b << blkLog));
    for (uint32_t p = threadIdx.x; p < blk / 2; p += 256) lds_put2(sm, p, src[p]);
  }
  __syncthreads();
  ntt_fwd_block_stages(sm, blkLog, b, logN, tw + ((uint64_t)t << logN), twp + ((uint64_t)t << logN), q);
  const uint64_t TN = (uint64_t)towers << logN;
  const uint64_t off = ((uint64_t)t << logN) + ((uint64_t)b << blkLog);
  for (uint32_t p = threadIdx.x; p < blk / 2; p += 256) {
    const ulonglong2 v = lds_get2(sm, p);
    pd_store_pair(ct, sk, sksh, out, k, TN, off + 2 * p, q, lead != 0,
                  make_ulonglong2(canon8(v.x, q), canon8(v.y, q)));
  }
}

size_t partial_decrypt_scratch_bytes(const Params& p, uint32_t towers, uint64_t K, double sigma) {
  if (!(sigma > 0.0) || p.logN == ntt_block_log(p.logN)) return 0;
  return K * (uint64_t)towers * p.N * sizeof(uint64_t);  // the noise between its two passes
}

void launch_partial_decrypt(const Params& p, const DeviceTables& dt, const DeviceKeys& dk, const uint64_t* ct,
                            uint64_t K, uint32_t towers, bool lead, uint64_t* out, void* scratch, double sigma,
                            const uint32_t key[8], uint64_t g0, hipStream_t s) {
  if (!K) return;
  if (towers < 1 || towers > p.L) throw Error{SHELFI_ERR_ARG, "partial decrypt: tower count out of range"};
  const uint64_t P = K * towers;
  if (!(sigma > 0.0)) {
    const uint64_t pairs = P * (p.N / 2), nb = (pairs + 255) / 256;
    if (nb > 0x7FFFFFFFull) throw Error{SHELFI_ERR_ARG, "partial decrypt batch too large"};
    hipLaunchKernelGGL(pd_plain_kernel, dim3((uint32_t)nb), dim3(256), 0, s, ct, dk.sk, dk.sk_sh, dt.tc, towers,
                       p.logN, pairs, lead ? 1 : 0, out);
    SHELFI_HIP(hipGetLastError());
    return;
  }
  PdNoise nz;
  for (int i = 0; i < 8; ++i) nz.key.k[i] = key[i];
  nz.g0 = g0;
  nz.sigma = sigma;
  const uint32_t blkLog = ntt_block_log(p.logN);
  const int logR = (int)(p.logN - blkLog);
  const uint64_t nbBlocks = P << logR;
  if (nbBlocks > 0x7FFFFFFFull) throw Error{SHELFI_ERR_ARG, "partial decrypt batch too large"};
  uint64_t* ebuf = reinterpret_cast<uint64_t*>(scratch);
  if (logR > 0) {
    const uint64_t nbCols = K * ((p.N >> logR) / 256);
#define PD_COLS(LR)                                                                                          \
  hipLaunchKernelGGL(pd_noise_cols<LR>, dim3((uint32_t)nbCols), dim3(256), 0, s, ebuf, towers, p.logN, dt.psi_rev, \
                     dt.psi_rev_sh, dt.tc, nz)
    switch (logR) {
      case 1: PD_COLS(1); break;
      case 2: PD_COLS(2); break;
      case 3: PD_COLS(3); break;
      case 4: PD_COLS(4); break;
      case 5: PD_COLS(5); break;
      case 6: PD_COLS(6); break;
      default: throw Error{SHELFI_ERR_ARG, "unsupported ring dimension"};
    }
#undef PD_COLS
    SHELFI_HIP(hipGetLastError());
  }
  if (logR > 0 && blkLog == 11 && dt.red_ok)
    hipLaunchKernelGGL((pd_blocks_ct<11, 3, 3, 3, 2>), dim3((uint32_t)nbBlocks), dim3(256), 0, s, ebuf, towers, p.logN,
                       dt.tw_fwd_blk, dt.tc, ct, dk.sk, dk.sk_sh, lead ? 1 : 0, out);
  else if (logR > 0 && blkLog == 12 && dt.red_ok)
    hipLaunchKernelGGL((pd_blocks_ct<12, 3, 3, 3, 3>), dim3((uint32_t)nbBlocks), dim3(256), 0, s, ebuf, towers, p.logN,
                       dt.tw_fwd_blk, dt.tc, ct, dk.sk, dk.sk_sh, lead ? 1 : 0, out);
  else
    hipLaunchKernelGGL(pd_blocks, dim3((uint32_t)nbBlocks), dim3(256), sizeof(uint64_t) << blkLog, s, ebuf, towers,
                       p.logN, (uint32_t)logR, dt.psi_rev, dt.psi_rev_sh, dt.tc, ct, dk.sk, dk.sk_sh, lead ? 1 : 0, out,
                       nz);
  SHELFI_HIP(hipGetLastError());
}

}  // namespace shelfi
