// poly.hip — EvalPoly's combine on gfx950: Paterson-Stockmeyer with four baby steps,
// p(x) = sum_g x^{4g} q_g(x), every giant-step product summed as ONE three-component tensor and relinearized once
// per output ciphertext.  With B_j = P_j (j = 1..nb), Gamma_g = P_{4g} (g = 1..ng) and the integer constants
// W_{g,j} of the plan (poly_plan.cpp), per ciphertext k, tower t and evaluation point, mod q_t:
//
//   q_{g,0} = W_{g,0} + sum_j W_{g,j} B_{j,0},   q_{g,1} = sum_j W_{g,j} B_{j,1}
//   d0 = q_{0,0} + sum_{g>=1} Gamma_{g,0} q_{g,0}
//   d1 = q_{0,1} + sum_{g>=1} (Gamma_{g,0} q_{g,1} + Gamma_{g,1} q_{g,0}),   d2 = sum_{g>=1} Gamma_{g,1} q_{g,1}
//   out[k] = (d0, d1) + KeySwitch(d2)         -- keyswitch.hip's launch_key_switch over the chain's K ciphertexts
//
//   poly_combine_kernel<true>   wsum_tensor_intt_kernel's place in the chain and its geometry
//   poly_combine_kernel<false>  ng = 0: q_0 alone, two components, no LDS and no key switch
//   launch_key_switch           keyswitch.hip's, unchanged
//
// Every operand is read in place at its own polynomial stride (its stored towers times N): the powers come out of
// different numbers of rescales, and dropping towers of an RNS ciphertext is only a stride.
#include <hip/hip_runtime.h>

#include "dot_dev.h"
#include "shelfi_internal.h"

namespace shelfi {

// No mid-run fold.  d1 starts from q_{0,1}'s unreduced sum (kPolyMaxBabies products of canonical residues) and
// takes two products a giant; d0 starts from a constant below q and q_{0,0}'s kPolyMaxBabies products and takes
// one a giant; a q_{g,.} is a constant and kPolyMaxBabies products.  The longest run is d1's 3 + 2 * 7 = 17
// products, each <= (q - 1)^2: dot_dev.h's fold interval is at least 128 ciphertexts of two products each for
// every tower the library builds (b <= 60 bits), so one dot_red128 per accumulator at the end is exact.
// dot_fold_interval's bound in PRODUCTS (it returns ciphertexts of two products each), as a constant expression:
// the products of canonical residues an accumulator that starts below q takes without wrapping, on a b-bit tower.
constexpr uint64_t poly_fold_products(int b) {
  const int e = 128 - 2 * b < 1 ? 1 : (128 - 2 * b > 32 ? 32 : 128 - 2 * b);
  return 1ull << e;
}
constexpr int kPolyLongestRun = kPolyMaxBabies + 2 * kPolyMaxGiants;  // d1's: q_{0,1}'s products, two a giant
static_assert(kPolyLongestRun == 17 && (uint64_t)kPolyLongestRun <= poly_fold_products(60),
              "poly_combine_kernel folds its accumulators once, at the end: its longest run of products must stay "
              "within the fold interval of the widest tower the library builds (60 bits: 256 products)");

// By value in the kernel arguments.  b[j - 1] = P_j, g[i - 1] = P_{4i}: the first ciphertext of the chain;
// bt / gt: the towers each is stored with.
struct PolyArgs {
  const uint64_t* b[kPolyMaxBabies];
  const uint64_t* g[kPolyMaxGiants];
  uint32_t bt[kPolyMaxBabies];
  uint32_t gt[kPolyMaxGiants];
};

// One workgroup per (k, tower, NTT block), 256 threads, 16-byte pairs, k FASTEST in blockIdx.x: the workgroups in
// flight together share a tower and with it the (ng + 1) x 4 constants wt[t] (uniform: scalar loads).  A thread
// walks its pairs one after another; a pair's 2 nb + 2 ng loads are issued before any is used (at most 20 x 16
// bytes in flight a thread).  q_{g,.} is reduced to [0, q) before it meets Gamma_g, so every product that enters
// d0 / d1 / d2 is one of canonical residues.  KS: d0, d1 -> out, d2 -> d2e and, through the first inverse
// stages in LDS, d2c -- exactly wsum_tensor_intt_kernel's hand-off.
template <bool KS>
__global__ __launch_bounds__(256) void poly_combine_kernel(const PolyArgs a, uint32_t nb, uint32_t ng, uint32_t K,
                                                           uint32_t Ll, uint32_t logN, uint32_t blkLog,
                                                           const uint64_t* __restrict__ wt,  // [Ll][ng + 1][4]
                                                           const uint64_t* __restrict__ itw,
                                                           const uint64_t* __restrict__ itwp,
                                                           const TowerConst* __restrict__ tq,
                                                           uint64_t* __restrict__ out, uint64_t* __restrict__ d2e,
                                                           uint64_t* __restrict__ d2c) {
  extern __shared__ __attribute__((aligned(16))) uint64_t sm[];
  const uint32_t N = 1u << logN, blk = 1u << blkLog, sh = logN - blkLog;
  const uint64_t k = blockIdx.x % K;
  const uint32_t tb = blockIdx.x / K;  // t * 2^sh + b
  const uint32_t t = tb >> sh, b = tb & ((1u << sh) - 1);
  const TowerConst c = tq[t];
  const uint64_t* W = wt + (uint64_t)t * (ng + 1) * 4;
  const uint64_t off = ((uint64_t)t << logN) + ((uint64_t)b << blkLog);
  const uint64_t poly = (uint64_t)Ll << logN;
  const uint64_t io = k * 2 * poly + off;
  const uint64_t id = ((k * Ll + t) << logN) + ((uint64_t)b << blkLog);
  ulonglong2* O0 = reinterpret_cast<ulonglong2*>(out + io);
  ulonglong2* O1 = reinterpret_cast<ulonglong2*>(out + io + poly);
  ulonglong2* E2 = KS ? reinterpret_cast<ulonglong2*>(d2e + id) : nullptr;
  for (uint32_t p = threadIdx.x; p < blk / 2; p += 256) {
    ulonglong2 b0[kPolyMaxBabies], b1[kPolyMaxBabies], g0[kPolyMaxGiants], g1[kPolyMaxGiants];
#pragma unroll
    for (int j = 0; j < kPolyMaxBabies; ++j)
      if (j < (int)nb) {
        const uint64_t bp = (uint64_t)a.bt[j] << logN;
        const uint64_t* s = a.b[j] + k * 2 * bp + off + 2u * p;
        b0[j] = ld_pair(s);
        b1[j] = ld_pair(s + bp);
      }
    if (KS) {
#pragma unroll
      for (int g = 0; g < kPolyMaxGiants; ++g)
        if (g < (int)ng) {
          const uint64_t gp = (uint64_t)a.gt[g] << logN;
          const uint64_t* s = a.g[g] + k * 2 * gp + off + 2u * p;
          g0[g] = ld_pair(s);
          g1[g] = ld_pair(s + gp);
        }
    }
    // q_g's two unreduced sums, for both residues of the pair
    const auto inner = [&](uint32_t g, du128& q0x, du128& q0y, du128& q1x, du128& q1y) {
      const uint64_t* w = W + 4 * g;
      q0x = q0y = w[0];
      q1x = q1y = 0;
#pragma unroll
      for (int j = 0; j < kPolyMaxBabies; ++j)
        if (j < (int)nb) {
          const uint64_t wj = w[1 + j];
          q0x += (du128)wj * b0[j].x;
          q0y += (du128)wj * b0[j].y;
          q1x += (du128)wj * b1[j].x;
          q1y += (du128)wj * b1[j].y;
        }
    };
    du128 d0x, d0y, d1x, d1y, d2x = 0, d2y = 0;
    inner(0, d0x, d0y, d1x, d1y);
    if (KS) {
#pragma unroll
      for (int g = 0; g < kPolyMaxGiants; ++g)
        if (g < (int)ng) {
          du128 ax, ay, bx, by;
          inner(g + 1, ax, ay, bx, by);
          const uint64_t q0x = dot_red128(ax, c), q0y = dot_red128(ay, c);
          const uint64_t q1x = dot_red128(bx, c), q1y = dot_red128(by, c);
          d0x += (du128)g0[g].x * q0x;
          d0y += (du128)g0[g].y * q0y;
          d1x += (du128)g0[g].x * q1x;
          d1x += (du128)g1[g].x * q0x;
          d1y += (du128)g0[g].y * q1y;
          d1y += (du128)g1[g].y * q0y;
          d2x += (du128)g1[g].x * q1x;
          d2y += (du128)g1[g].y * q1y;
        }
    }
    O0[p] = make_ulonglong2(dot_red128(d0x, c), dot_red128(d0y, c));
    O1[p] = make_ulonglong2(dot_red128(d1x, c), dot_red128(d1y, c));
    if (KS) {
      const ulonglong2 r2 = make_ulonglong2(dot_red128(d2x, c), dot_red128(d2y, c));
      E2[p] = r2;
      lds_put2(sm, p, r2);
    }
  }
  if (KS) {
    __syncthreads();
    ks_intt_block_out(sm, blkLog, b, logN, itw + (uint64_t)t * N, itwp + (uint64_t)t * N, c, d2c + id);
  }
}

void launch_poly_combine(const KsArgs* a, const DeviceTables& dtq, const DeviceTables* dte, const DeviceTables* dtf,
                         const uint64_t* evk, const uint64_t* evk_sh, const uint64_t* const* babies,
                         const uint32_t* baby_towers, uint32_t nb, const uint64_t* const* giants,
                         const uint32_t* giant_towers, uint32_t ng, const uint64_t* wt_dev, uint32_t Ll, uint32_t logN,
                         uint64_t k0, uint64_t kc, uint64_t* out, void* scratch, hipStream_t s) {
  if (!kc) return;
  if (nb < 1 || nb > (uint32_t)kPolyMaxBabies || ng > (uint32_t)kPolyMaxGiants || (ng && !a))
    throw Error{SHELFI_ERR_ARG, "EvalPoly: bad operand counts"};
  const uint32_t blkLog = ntt_block_log(logN), sh = logN - blkLog;
  const uint64_t blocks = (kc * Ll) << sh;
  if (blocks > 0x7FFFFFFFull) throw Error{SHELFI_ERR_ARG, "EvalPoly batch too large"};
  PolyArgs g{};
  for (uint32_t j = 0; j < nb; ++j) {
    if (baby_towers[j] < Ll) throw Error{SHELFI_ERR_ARG, "EvalPoly: an operand stored below the combine level"};
    g.bt[j] = baby_towers[j];
    g.b[j] = babies[j] + k0 * (2ull * baby_towers[j] << logN);
  }
  for (uint32_t i = 0; i < ng; ++i) {
    if (giant_towers[i] < Ll) throw Error{SHELFI_ERR_ARG, "EvalPoly: an operand stored below the combine level"};
    g.gt[i] = giant_towers[i];
    g.g[i] = giants[i] + k0 * (2ull * giant_towers[i] << logN);
  }
  uint64_t* o = out + k0 * (2ull * Ll << logN);
  if (!ng) {
    hipLaunchKernelGGL(poly_combine_kernel<false>, dim3((uint32_t)blocks), dim3(256), 0, s, g, nb, 0u, (uint32_t)kc, Ll,
                       logN, blkLog, wt_dev, nullptr, nullptr, dtq.tc, o, nullptr, nullptr);
    SHELFI_HIP(hipGetLastError());
    return;
  }
  const KsScratch ks = ks_scratch_layout(*a, kc, scratch);
  hipLaunchKernelGGL(poly_combine_kernel<true>, dim3((uint32_t)blocks), dim3(256), sizeof(uint64_t) << blkLog, s, g, nb,
                     ng, (uint32_t)kc, Ll, logN, blkLog, wt_dev, dtq.ipsi_rev, dtq.ipsi_rev_sh, a->tq, o, ks.d2e, ks.d2c);
  SHELFI_HIP(hipGetLastError());
  launch_key_switch(*a, dtq, *dte, dtf, evk, evk_sh, kc, o, scratch, s);
}

}  // namespace shelfi
