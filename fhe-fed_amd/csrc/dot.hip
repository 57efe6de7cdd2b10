// dot.hip — EvalInnerProduct on gfx950: sum_k a_k (x) b_k over K ciphertext pairs with ONE
// relinearization (PALISADE's EvalMultNoRelin + EvalAddMany + Relinearize as one device call).
//
//   c0 = sum_k a_k0 b_k0,  c1 = sum_k (a_k0 b_k1 + a_k1 b_k0),  c2 = sum_k a_k1 b_k1   (mod q_t)
//   out = (c0, c1) + KeySwitch(c2)      -- keyswitch.hip's launch_key_switch with K = 1
//
// Relinearization is linear, so this decrypts to what sum_k EvalMult(a_k, b_k) decrypts to, with one
// key switch instead of K.  What remains per ciphertext is a streaming pass (four polynomial reads per
// tower, two when a is b), split over S slices of the K ciphertexts so that a small K still fills the
// machine:
//   dot_partial_kernel      slice s -> canonical partial sums part[s][3][Ll][N]
//   dot_reduce_intt_kernel  sums the S partials; c0, c1 -> out, c2 -> d2e and, through the first
//                           inverse stages in LDS, d2c (ks_tensor_intt_kernel's place in the chain)
// Sums mod q_t are exact, so no output bit depends on S.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dot_dev.h"
#include "shelfi_internal.h"

namespace shelfi {

// Grid (512-coefficient block, tower, slice); one thread = 2 adjacent coefficients (16-byte loads), the
// tower block-uniform so its constants sit in SGPRs (wavg_kernel's arrangement).  The workgroup walks
// ciphertexts [k0, k1) of its slice, U of them loaded before any is used (8 16-byte loads in flight per
// thread), accumulates the three sums in 128-bit accumulators with no reduction, and folds them every
// dot_fold_interval ciphertexts and at the end.  Nothing here needs TowerConst::red_ok: 30-bit chains run
// the same code.  SQUARE (a is b): each ciphertext is read once.
template <bool SQUARE>
__global__ __launch_bounds__(256) void dot_partial_kernel(const uint64_t* __restrict__ a,
                                                          const uint64_t* __restrict__ b, uint64_t K, uint32_t S,
                                                          uint32_t Ll, uint32_t logN,
                                                          const TowerConst* __restrict__ tq,
                                                          uint64_t* __restrict__ part) {
  constexpr int U = SQUARE ? 4 : 2;
  const uint32_t t = blockIdx.y, s = blockIdx.z;
  const TowerConst c = tq[t];
  const uint64_t k0 = (uint64_t)s * K / S, k1 = (uint64_t)(s + 1) * K / S;  // balanced: no empty slice (S <= K)
  const uint64_t G = dot_fold_interval(c.q);
  const uint64_t e = (uint64_t)blockIdx.x * 512 + 2u * threadIdx.x;
  const uint64_t poly = (uint64_t)Ll << logN, ctw = 2 * poly;
  const uint64_t off = ((uint64_t)t << logN) + e;
  du128 c0x = 0, c0y = 0, c1x = 0, c1y = 0, c2x = 0, c2y = 0;
  const auto take = [&](const ulonglong2& a0, const ulonglong2& a1, const ulonglong2& b0, const ulonglong2& b1) {
    c0x += (du128)a0.x * b0.x;
    c0y += (du128)a0.y * b0.y;
    c2x += (du128)a1.x * b1.x;
    c2y += (du128)a1.y * b1.y;
    if (SQUARE) {
      const du128 mx = (du128)a0.x * a1.x, my = (du128)a0.y * a1.y;
      c1x += mx + mx;
      c1y += my + my;
    } else {
      c1x += (du128)a0.x * b1.x;
      c1x += (du128)a1.x * b0.x;
      c1y += (du128)a0.y * b1.y;
      c1y += (du128)a1.y * b0.y;
    }
  };
  uint64_t k = k0;
  while (k < k1) {
    const uint64_t ke = min(k1, k + G);
    for (; k + U <= ke; k += U) {
      ulonglong2 a0[U], a1[U], b0[U], b1[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const uint64_t i = (k + u) * ctw + off;
        a0[u] = ld_pair(a + i);
        a1[u] = ld_pair(a + i + poly);
        if (!SQUARE) {
          b0[u] = ld_pair(b + i);
          b1[u] = ld_pair(b + i + poly);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) take(a0[u], a1[u], SQUARE ? a0[u] : b0[u], SQUARE ? a1[u] : b1[u]);
    }
    for (; k < ke; ++k) {
      const uint64_t i = k * ctw + off;
      const ulonglong2 a0 = ld_pair(a + i), a1 = ld_pair(a + i + poly);
      const ulonglong2 b0 = SQUARE ? a0 : ld_pair(b + i), b1 = SQUARE ? a1 : ld_pair(b + i + poly);
      take(a0, a1, b0, b1);
    }
    c0x = dot_red128(c0x, c);
    c0y = dot_red128(c0y, c);
    c1x = dot_red128(c1x, c);
    c1y = dot_red128(c1y, c);
    c2x = dot_red128(c2x, c);
    c2y = dot_red128(c2y, c);
  }
  uint64_t* __restrict__ o = part + (uint64_t)s * 3 * poly + off;
  *reinterpret_cast<ulonglong2*>(o) = make_ulonglong2((uint64_t)c0x, (uint64_t)c0y);
  *reinterpret_cast<ulonglong2*>(o + poly) = make_ulonglong2((uint64_t)c1x, (uint64_t)c1y);
  *reinterpret_cast<ulonglong2*>(o + 2 * poly) = make_ulonglong2((uint64_t)c2x, (uint64_t)c2y);
}

// One workgroup per (tower, NTT block), ks_tensor_intt_kernel's geometry with K = 1: dot_reduce_block on
// part [S][3][Ll][N].
__global__ __launch_bounds__(256) void dot_reduce_intt_kernel(const uint64_t* __restrict__ part, uint32_t S,
                                                              uint32_t Ll, uint32_t logN, uint32_t blkLog,
                                                              const uint64_t* __restrict__ itw,
                                                              const uint64_t* __restrict__ itwp,
                                                              const TowerConst* __restrict__ tq,
                                                              uint64_t* __restrict__ out,
                                                              uint64_t* __restrict__ d2e,
                                                              uint64_t* __restrict__ d2c) {
  extern __shared__ __attribute__((aligned(16))) uint64_t sm[];
  const uint32_t sh = logN - blkLog;
  const uint32_t t = blockIdx.x >> sh, b = blockIdx.x & ((1u << sh) - 1);
  const uint64_t poly = (uint64_t)Ll << logN;
  dot_reduce_block(sm, part, part + poly, 3 * poly, part + 2 * poly, 3 * poly, S, t, b, logN, blkLog, itw, itwp, tq[t], out,
                   out + poly, d2e, d2c);
}

// scratch: the key switch's for one ciphertext (rounded up to 64 bytes) | part [S][3][Ll][N]
static size_t dot_ks_bytes(const KsArgs& a) {
  return (ks_scratch_bytes(a.Ll, a.kP, a.dn, a.alpha, 1u << a.logN, 1) + 63) & ~(size_t)63;
}
size_t dot_scratch_bytes(const KsArgs& a, uint32_t S) {
  return dot_ks_bytes(a) + ((size_t)S * 3 * a.Ll << a.logN) * 8;
}

uint32_t dot_slices(uint64_t K, uint64_t slice_cts) {
  const uint64_t per = std::max<uint64_t>(1, slice_cts);
  return (uint32_t)std::min<uint64_t>(kDotMaxSlices, K / per + (K % per ? 1 : 0));
}

void launch_dot(const KsArgs& a, const DeviceTables& dtq, const DeviceTables& dte, const DeviceTables* dtf,
                const uint64_t* evk, const uint64_t* evk_sh, const uint64_t* x, const uint64_t* y, uint64_t K,
                uint32_t S, uint64_t* out, void* scratch, hipStream_t s) {
  if (!K) return;
  if (a.logN < 9) throw Error{SHELFI_ERR_ARG, "EvalInnerProduct: unsupported ring dimension"};
  if (S < 1 || S > (uint32_t)kDotMaxSlices || S > K) throw Error{SHELFI_ERR_ARG, "EvalInnerProduct: bad slice count"};
  uint64_t* part = reinterpret_cast<uint64_t*>(static_cast<char*>(scratch) + dot_ks_bytes(a));
  const dim3 grid(1u << (a.logN - 9), a.Ll, S);
  if (x == y)
    hipLaunchKernelGGL(dot_partial_kernel<true>, grid, dim3(256), 0, s, x, y, K, S, a.Ll, a.logN, a.tq, part);
  else
    hipLaunchKernelGGL(dot_partial_kernel<false>, grid, dim3(256), 0, s, x, y, K, S, a.Ll, a.logN, a.tq, part);
  SHELFI_HIP(hipGetLastError());
  const uint32_t blkLog = ntt_block_log(a.logN), sh = a.logN - blkLog;
  const KsScratch ks = ks_scratch_layout(a, 1, scratch);
  hipLaunchKernelGGL(dot_reduce_intt_kernel, dim3(a.Ll << sh), dim3(256), sizeof(uint64_t) << blkLog, s, part, S, a.Ll,
                     a.logN, blkLog, dtq.ipsi_rev, dtq.ipsi_rev_sh, a.tq, out, ks.d2e, ks.d2c);
  SHELFI_HIP(hipGetLastError());
  launch_key_switch(a, dtq, dte, dtf, evk, evk_sh, 1, out, scratch, s);
}

}  // namespace shelfi
