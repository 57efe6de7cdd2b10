// keygen.hip — key generation: ternary s, Gaussian e, uniform a.
//
// Kernels:
//   keygen_sample_kernel         s, e and a from the ChaCha20 stream
//   keygen_combine_kernel        b = e - a*s
//   keygen_chain_combine_kernel  the threshold key chain's step: b = prev.b + e - a*s over prev.a (mkhe.cpp:282)
#include <hip/hip_runtime.h>

#include "dev_common.h"
#include "shelfi_internal.h"

namespace shelfi {

// --------------------------------------------------------------- keygen ----
// s ternary (nonce 2<<56, words [0,N)), e Gaussian (words [N,2N)), a_t uniform
// (nonce (2<<56)|(1+t), word pair (2j, 2j+1) -> 128-bit value mod q_t).
__global__ __launch_bounds__(256) void keygen_sample_kernel(uint32_t logN, uint32_t L,
                                                            const TowerConst* __restrict__ tcs,
                                                            const uint64_t* __restrict__ cdt, int T,
                                                            Key8 key, uint64_t* __restrict__ se,
                                                            uint64_t* __restrict__ a_out) {
  const uint32_t N = 1u << logN;
  const uint32_t gid = blockIdx.x * 256 + threadIdx.x;
  if (gid >= (N >> 3)) return;
  const uint32_t j0 = gid * 8;
  const uint64_t nonce = 2ull << 56;
  uint64_t rs[8], re[8];
  chacha20_block(key, j0 >> 3, nonce, rs);
  chacha20_block(key, (N >> 3) + (j0 >> 3), nonce, re);
  int64_t sv[8], ev[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    sv[u] = ternary_sample(rs[u]);
    ev[u] = gauss_sample(re[u], cdt, T);
  }
  for (uint32_t t = 0; t < L; ++t) {
    const TowerConst c = tcs[t];
    uint64_t ra[16];
    chacha20_block(key, j0 >> 2, nonce | (1 + t), ra);
    chacha20_block(key, (j0 >> 2) + 1, nonce | (1 + t), ra + 8);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      se[((uint64_t)0 * L + t) * N + j0 + u] = mod_signed_dev(sv[u], c);
      se[((uint64_t)1 * L + t) * N + j0 + u] = mod_signed_dev(ev[u], c);
      const uint64_t lo = ra[2 * u], hi = ra[2 * u + 1];
      a_out[(uint64_t)t * N + j0 + u] =
          addmod(shoup_mul(red64(hi, c.q, c.one_shoup), c.r64, c.r64_shoup, c.q),
                 red64(lo, c.q, c.one_shoup), c.q);
    }
  }
}

// sk = NTT(s); b = NTT(e) - a * NTT(s)
__global__ __launch_bounds__(256) void keygen_combine_kernel(const uint64_t* __restrict__ se,
                                                             uint32_t logN, uint32_t L,
                                                             const TowerConst* __restrict__ tcs,
                                                             uint64_t* __restrict__ sk,
                                                             uint64_t* __restrict__ pk) {
  const uint64_t LN = (uint64_t)L << logN;
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= LN) return;
  const uint32_t t = (uint32_t)(e >> logN);
  const TowerConst c = tcs[t];
  const uint64_t s = se[e], er = se[LN + e], a = pk[LN + e];
  sk[e] = s;
  pk[e] = submod(er, mulmod_generic(a, s, c), c.q);
}

size_t keygen_scratch_bytes(const Params& p) { return 2ull * p.L * p.N * sizeof(uint64_t); }

// s and e sampled into se [2][L][N] and transformed (NTT(s), NTT(e)); the uniform a goes to a_out [L][N]
static void keygen_sample_ntt(const Params& p, const DeviceTables& dt, const uint32_t key[8], uint64_t* se,
                              uint64_t* a_out, hipStream_t s) {
  Key8 k8;
  for (int i = 0; i < 8; ++i) k8.k[i] = key[i];
  const uint32_t th = p.N / 8;
  hipLaunchKernelGGL(keygen_sample_kernel, dim3((th + 255) / 256), dim3(256), 0, s, p.logN, p.L,
                     dt.tc, dt.cdt, dt.cdt_len, k8, se, a_out);
  SHELFI_HIP(hipGetLastError());
  launch_ntt(se, 2ull * p.L, p.L, p.logN, false, dt, s);
}

void launch_keygen(const Params& p, const DeviceTables& dt, const uint32_t key[8], uint64_t* sk,
                   uint64_t* pk, void* scratch, hipStream_t s) {
  uint64_t* se = reinterpret_cast<uint64_t*>(scratch);
  const uint64_t LN = (uint64_t)p.L * p.N;
  keygen_sample_ntt(p, dt, key, se, pk + LN, s);
  hipLaunchKernelGGL(keygen_combine_kernel, dim3((uint32_t)((LN + 255) / 256)), dim3(256), 0, s,
                     se, p.logN, p.L, dt.tc, sk, pk);
  SHELFI_HIP(hipGetLastError());
}

// One step of the threshold key chain (mkhe.cpp:282 MultipartyKeyGen): sk = NTT(s);
// b = prev.b + NTT(e) - a * NTT(s) with a = prev.a (prev [2][L][N]: b, a).
__global__ __launch_bounds__(256) void keygen_chain_combine_kernel(const uint64_t* __restrict__ se, uint32_t logN,
                                                                   uint32_t L, const TowerConst* __restrict__ tcs,
                                                                   const uint64_t* __restrict__ prev,
                                                                   uint64_t* __restrict__ sk,
                                                                   uint64_t* __restrict__ pk) {
  const uint64_t LN = (uint64_t)L << logN;
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= LN) return;
  const uint32_t t = (uint32_t)(e >> logN);
  const TowerConst c = tcs[t];
  const uint64_t s = se[e], er = se[LN + e], a = prev[LN + e];
  sk[e] = s;
  pk[e] = addmod(prev[e], submod(er, mulmod_generic(a, s, c), c.q), c.q);
  pk[LN + e] = a;
}

// s, e from keygen's stream ([0, N) and [N, 2N) of nonce 2 << 56); the a it would draw lands in the
// scratch and is dropped
size_t keygen_chain_scratch_bytes(const Params& p) { return 3ull * p.L * p.N * sizeof(uint64_t); }

void launch_keygen_chain(const Params& p, const DeviceTables& dt, const uint32_t key[8], const uint64_t* prev_pk,
                         uint64_t* sk, uint64_t* pk, void* scratch, hipStream_t s) {
  uint64_t* se = reinterpret_cast<uint64_t*>(scratch);
  const uint64_t LN = (uint64_t)p.L * p.N;
  keygen_sample_ntt(p, dt, key, se, se + 2 * LN, s);
  hipLaunchKernelGGL(keygen_chain_combine_kernel, dim3((uint32_t)((LN + 255) / 256)), dim3(256), 0, s, se, p.logN,
                     p.L, dt.tc, prev_pk, sk, pk);
  SHELFI_HIP(hipGetLastError());
}

}  // namespace shelfi
