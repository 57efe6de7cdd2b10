// ntt.hip — the generic negacyclic NTT / INTT over [P][N] polynomials, 2 passes (register
// columns + LDS blocks).
//
// Kernels:
//   ntt_fwd_cols, ntt_inv_cols        the top logN - BL stages on register columns
//   ntt_fwd_blocks, ntt_inv_blocks    the stages inside contiguous blocks, run-time shape
//                                     (ntt_inv_blocks: transform_dev.h; its NoFuse form is emitted here)
//   ntt_fwd_blocks_ct, ntt_inv_blocks_ct  the same at compile-time shape over per-block twiddle slices
#include <hip/hip_runtime.h>

#include "dev_common.h"
#include "shelfi_internal.h"
#include "transform_dev.h"

namespace shelfi {

// ------------------------------------------------------------------- NTT ----
// Forward (Cooley-Tukey, natural -> bit-reversed), stage m (= 2^s) pairs
// (j, j + N/2m) with twiddle psi_rev[m + j/(N/m)].  The first LOGR stages pair
// elements R = 2^LOGR apart in the top bits: each thread holds one column of R
// elements (stride N/R) in registers, all twiddles wave-uniform.  The remaining
// stages act inside contiguous blocks of N/R elements, staged in LDS.
template <int LOGR>
__global__ __launch_bounds__(256) void ntt_fwd_cols(uint64_t* __restrict__ polys, uint32_t L,
                                                    uint32_t logN, const uint64_t* __restrict__ tw,
                                                    const uint64_t* __restrict__ twp,
                                                    const TowerConst* __restrict__ tcs) {
  constexpr int R = 1 << LOGR;
  const uint32_t N = 1u << logN;
  const uint32_t BLK = N >> LOGR;
  const uint32_t bpp = BLK / 256;
  const uint64_t poly = blockIdx.x / bpp;
  const uint32_t col = (blockIdx.x % bpp) * 256 + threadIdx.x;
  const uint32_t t = (uint32_t)(poly % L);
  const uint64_t q = tcs[t].q;
  const uint64_t* __restrict__ w = tw + (uint64_t)t * N;
  const uint64_t* __restrict__ wp = twp + (uint64_t)t * N;
  uint64_t* __restrict__ a = polys + poly * N + col;
  uint64_t x[R];
#pragma unroll
  for (int r = 0; r < R; ++r) x[r] = a[(uint64_t)r * BLK];
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
  // lazy values in [0, 8q): the blocks pass that follows canonicalises
#pragma unroll
  for (int r = 0; r < R; ++r) a[(uint64_t)r * BLK] = x[r];
}

// Blocks pass, stages s = sstart .. logN-1 on contiguous blocks of 2^(logN-sstart).
__global__ __launch_bounds__(256) void ntt_fwd_blocks(uint64_t* __restrict__ polys, uint32_t L,
                                                      uint32_t logN, uint32_t sstart,
                                                      const uint64_t* __restrict__ tw,
                                                      const uint64_t* __restrict__ twp,
                                                      const TowerConst* __restrict__ tcs) {
  extern __shared__ __attribute__((aligned(16))) uint64_t sm[];
  const uint32_t N = 1u << logN, blkLog = logN - sstart, blk = 1u << blkLog;
  const uint32_t nb = 1u << sstart;
  const uint64_t poly = blockIdx.x >> sstart;
  const uint32_t b = blockIdx.x & (nb - 1);
  const uint32_t t = (uint32_t)(poly % L);
  const uint64_t q = tcs[t].q;
  uint64_t* __restrict__ a = polys + poly * N + ((uint64_t)b << blkLog);
  for (uint32_t p = threadIdx.x; p < blk / 2; p += 256)
    lds_put2(sm, p, reinterpret_cast<const ulonglong2*>(a)[p]);
  __syncthreads();
  ntt_fwd_block_stages(sm, blkLog, b, logN, tw + (uint64_t)t * N, twp + (uint64_t)t * N, q);
  for (uint32_t p = threadIdx.x; p < blk / 2; p += 256) {
    const ulonglong2 v = lds_get2(sm, p);
    reinterpret_cast<ulonglong2*>(a)[p] = make_ulonglong2(canon8(v.x, q), canon8(v.y, q));
  }
}

template <int LOGR>
__global__ __launch_bounds__(256) void ntt_inv_cols(uint64_t* __restrict__ polys, uint32_t L,
                                                    uint32_t logN, const uint64_t* __restrict__ tw,
                                                    const uint64_t* __restrict__ twp,
                                                    const TowerConst* __restrict__ tcs) {
  constexpr int R = 1 << LOGR;
  const uint32_t N = 1u << logN;
  const uint32_t BLK = N >> LOGR;
  const uint32_t bpp = BLK / 256;
  const uint64_t poly = blockIdx.x / bpp;
  const uint32_t col = (blockIdx.x % bpp) * 256 + threadIdx.x;
  const uint32_t t = (uint32_t)(poly % L);
  const TowerConst& c = tcs[t];
  const uint64_t q = c.q;
  const uint64_t* __restrict__ w = tw + (uint64_t)t * N;
  const uint64_t* __restrict__ wp = twp + (uint64_t)t * N;
  uint64_t* __restrict__ a = polys + poly * N + col;
  uint64_t x[R];
#pragma unroll
  for (int r = 0; r < R; ++r) x[r] = a[(uint64_t)r * BLK];
#pragma unroll
  for (int v = 0; v < LOGR; ++v) {
    const int tr = 1 << v, h = R >> (v + 1);
#pragma unroll
    for (int i = 0; i < h; ++i) {
      const uint64_t W = w[h + i], Wp = wp[h + i];
#pragma unroll
      for (int jj = 0; jj < tr; ++jj) {
        const int r0 = 2 * i * tr + jj, r1 = r0 + tr;
        if (gs_in8<true>(v, jj))  // inputs below 8q (ntt_inv_blocks_dec_ct leaves sums < 8q)
          gs_bfly_b<true>(x[r0], x[r1], W, Wp, q, c.n8q);
        else
          gs_bfly_b<false>(x[r0], x[r1], W, Wp, q, c.n8q);
      }
    }
  }
  const uint64_t ni = c.ninv, nip = c.ninv_shoup;
#pragma unroll
  for (int r = 0; r < R; ++r) a[(uint64_t)r * BLK] = canon4(shoup_lazy(x[r], ni, nip, q), q);
}

#define NTT_DISPATCH(LOGRV, KERNEL, ...)                                                   \
  switch (LOGRV) {                                                                       \
    case 1: hipLaunchKernelGGL(KERNEL<1>, __VA_ARGS__); break;                           \
    case 2: hipLaunchKernelGGL(KERNEL<2>, __VA_ARGS__); break;                           \
    case 3: hipLaunchKernelGGL(KERNEL<3>, __VA_ARGS__); break;                           \
    case 4: hipLaunchKernelGGL(KERNEL<4>, __VA_ARGS__); break;                           \
    case 5: hipLaunchKernelGGL(KERNEL<5>, __VA_ARGS__); break;                           \
    case 6: hipLaunchKernelGGL(KERNEL<6>, __VA_ARGS__); break;                           \
    default: throw Error{SHELFI_ERR_ARG, "unsupported ring dimension"};                  \
  }

// launch_ntt's block passes at compile-time shape (rings with a columns pass whose blocks are
// 2^11 or 2^12 elements and every q >= 2^40), in place over the per-block twiddle slices:
// forward after ntt_fwd_cols (inputs < 8q, canonical outputs), inverse before ntt_inv_cols
// (canonical inputs, lazy outputs below 8q).  A workgroup reads its whole block in the first
// chunk, before any of its writes.
template <int BL, int K1, int K2, int K3, int K4>
__global__ __launch_bounds__(256) void ntt_fwd_blocks_ct(uint64_t* polys, uint32_t L, uint32_t logN,
                                                         const ulonglong2* __restrict__ twb,
                                                         const TowerConst* __restrict__ tcs) {
  __shared__ __attribute__((aligned(16))) uint64_t sm[lpad_size(BL)];
  const uint32_t sh = logN - BL;
  const uint64_t poly = blockIdx.x >> sh;
  const uint32_t b = blockIdx.x & ((1u << sh) - 1);
  const uint32_t t = (uint32_t)(poly % L);
  const TowerConst& c = tcs[t];
  uint64_t* base = polys + (poly << logN) + ((uint64_t)b << BL);
  fwd_block_pass_ct<BL, K1, K2, K3, K4>(base, twb + ((uint64_t)t << logN) + ((uint64_t)b << BL), c.q, c.n8q, sm,
                                        [&](uint32_t j0, auto& x) {
#pragma unroll
                                          for (int m = 0; m < (1 << K4); m += 2)
                                            *reinterpret_cast<ulonglong2*>(base + j0 + m) =
                                                make_ulonglong2(red_any(x[m], c), red_any(x[m + 1], c));
                                        });
}
template <int BL, int K1, int K2, int K3, int K4>
__global__ __launch_bounds__(256) void ntt_inv_blocks_ct(uint64_t* polys, uint32_t L, uint32_t logN,
                                                         const ulonglong2* __restrict__ twb,
                                                         const TowerConst* __restrict__ tcs) {
  static_assert(K1 + K2 + K3 + K4 == BL, "chunk plan must cover the block");
  __shared__ __attribute__((aligned(16))) uint64_t sm[lpad_size(BL)];
  const uint32_t sh = logN - BL;
  const uint64_t poly = blockIdx.x >> sh;
  const uint32_t b = blockIdx.x & ((1u << sh) - 1);
  const uint32_t t = (uint32_t)(poly % L);
  const uint64_t q = tcs[t].q, n8q = tcs[t].n8q;
  uint64_t* base = polys + (poly << logN) + ((uint64_t)b << BL);
  const ulonglong2* __restrict__ tb = twb + ((uint64_t)t << logN) + ((uint64_t)b << BL);
  const auto lds_ld = [&](uint32_t, uint32_t pj) { return sm[pj]; };
  inv_chunk_ct<BL, 0, K1, false>(tb, q, n8q, [&](uint32_t j, uint32_t) { return base[j]; },
                                 [&](int, uint32_t, uint32_t pj0, auto& x) {
#pragma unroll
                                   for (int m = 0; m < (1 << K1); ++m) sm[pj0 + lofs<1>(m)] = x[m];
                                 });
  __syncthreads();
  inv_chunk_ct<BL, K1, K2, true>(tb, q, n8q, lds_ld, [&](int, uint32_t, uint32_t pj0, auto& x) {
#pragma unroll
    for (int m = 0; m < (1 << K2); ++m) sm[pj0 + lofs<(1 << K1)>(m)] = x[m];
  });
  __syncthreads();
  inv_chunk_ct<BL, K1 + K2, K3, true>(tb, q, n8q, lds_ld, [&](int, uint32_t, uint32_t pj0, auto& x) {
#pragma unroll
    for (int m = 0; m < (1 << K3); ++m) sm[pj0 + lofs<(1 << (K1 + K2))>(m)] = x[m];
  });
  __syncthreads();
  inv_chunk_ct<BL, BL - K4, K4, true>(tb, q, n8q, lds_ld, [&](int, uint32_t j0, uint32_t, auto& x) {
#pragma unroll
    for (int m = 0; m < (1 << K4); ++m) base[j0 + (m << (BL - K4))] = x[m];
  });
}

template __global__ void ntt_inv_blocks<NoFuse>(uint64_t*, uint32_t, uint32_t, uint32_t, const uint64_t*,
                                                const uint64_t*, const TowerConst*, int, const uint64_t*,
                                                const uint64_t*, const uint64_t*, int, uint32_t, NoFuse);

void launch_ntt(uint64_t* polys, uint64_t P, uint32_t L, uint32_t logN, bool inverse,
                const DeviceTables& dt, hipStream_t s) {
  if (!P) return;
  const uint32_t N = 1u << logN;
  const uint32_t blkLog = ntt_block_log(logN);
  const int logR = (int)(logN - blkLog);
  const uint32_t blk = 1u << blkLog;
  const size_t lds = (size_t)blk * sizeof(uint64_t);
  const uint64_t nbBlocks = P << logR;
  const uint64_t nbCols = P * ((N >> logR) / 256);
  if (nbBlocks > 0x7FFFFFFFull || nbCols > 0x7FFFFFFFull)
    throw Error{SHELFI_ERR_ARG, "NTT batch too large"};
  if (!inverse) {
    if (logR > 0) {
      NTT_DISPATCH(logR, ntt_fwd_cols, dim3((uint32_t)nbCols), dim3(256), 0, s, polys, L, logN,
                   dt.psi_rev, dt.psi_rev_sh, dt.tc);
    }
    if (logR > 0 && blkLog == 11 && dt.red_ok)
      hipLaunchKernelGGL((ntt_fwd_blocks_ct<11, 3, 3, 3, 2>), dim3((uint32_t)nbBlocks), dim3(256), 0, s, polys, L,
                         logN, dt.tw_fwd_blk, dt.tc);
    else if (logR > 0 && blkLog == 12 && dt.red_ok)
      hipLaunchKernelGGL((ntt_fwd_blocks_ct<12, 3, 3, 3, 3>), dim3((uint32_t)nbBlocks), dim3(256), 0, s, polys, L,
                         logN, dt.tw_fwd_blk, dt.tc);
    else
      hipLaunchKernelGGL(ntt_fwd_blocks, dim3((uint32_t)nbBlocks), dim3(256), lds, s, polys, L,
                         logN, (uint32_t)logR, dt.psi_rev, dt.psi_rev_sh, dt.tc);
  } else {
    if (logR > 0 && blkLog == 11 && dt.red_ok)
      hipLaunchKernelGGL((ntt_inv_blocks_ct<11, 2, 3, 3, 3>), dim3((uint32_t)nbBlocks), dim3(256), 0, s, polys, L,
                         logN, dt.tw_inv_blk, dt.tc);
    else if (logR > 0 && blkLog == 12 && dt.red_ok)
      hipLaunchKernelGGL((ntt_inv_blocks_ct<12, 3, 3, 3, 3>), dim3((uint32_t)nbBlocks), dim3(256), 0, s, polys, L,
                         logN, dt.tw_inv_blk, dt.tc);
    else
      hipLaunchKernelGGL(ntt_inv_blocks<>, dim3((uint32_t)nbBlocks), dim3(256), lds, s, polys, L,
                         logN, blkLog, dt.ipsi_rev, dt.ipsi_rev_sh, dt.tc, logR == 0 ? 1 : 0,
                         (const uint64_t*)nullptr, (const uint64_t*)nullptr, (const uint64_t*)nullptr, 0, L,
                         NoFuse{});
    if (logR > 0) {
      NTT_DISPATCH(logR, ntt_inv_cols, dim3((uint32_t)nbCols), dim3(256), 0, s, polys, L, logN,
                   dt.ipsi_rev, dt.ipsi_rev_sh, dt.tc);
    }
  }
  SHELFI_HIP(hipGetLastError());
}

// The register-columns pass alone (the first logN - BL forward stages / the last inverse
// stages), for callers that fuse their own blocks pass (keyswitch.hip).  No-op when the
// whole transform is one block (N <= 2^BL).
void launch_ntt_cols(uint64_t* polys, uint64_t P, uint32_t L, uint32_t logN, bool inverse,
                     const DeviceTables& dt, hipStream_t s) {
  const uint32_t N = 1u << logN;
  const int logR = (int)(logN - ntt_block_log(logN));
  if (!P || logR == 0) return;
  const uint64_t nbCols = P * ((N >> logR) / 256);
  if (nbCols > 0x7FFFFFFFull) throw Error{SHELFI_ERR_ARG, "NTT batch too large"};
  if (!inverse)
    NTT_DISPATCH(logR, ntt_fwd_cols, dim3((uint32_t)nbCols), dim3(256), 0, s, polys, L, logN, dt.psi_rev,
                 dt.psi_rev_sh, dt.tc)
  else
    NTT_DISPATCH(logR, ntt_inv_cols, dim3((uint32_t)nbCols), dim3(256), 0, s, polys, L, logN, dt.ipsi_rev,
                 dt.ipsi_rev_sh, dt.tc)
  SHELFI_HIP(hipGetLastError());
}

}  // namespace shelfi
