// wsum.hip — EvalLinearWSum with ENCRYPTED weights on gfx950: out[k] = sum_c w_c (x) u_{c,k} over C learners'
// update batches u_c [K][2][Lu][N] and weight batches w_c [Kw][2][Ll][N] (Kw = 1: one weight ciphertext for a
// learner's whole update; Kw = K: one per update ciphertext), with ONE key switch per output ciphertext:
//
//   c0 = sum_c w0 u_{c,k,0},  c1 = sum_c (w0 u_{c,k,1} + w1 u_{c,k,0}),  c2 = sum_c w1 u_{c,k,1}   (mod q_t)
//   out[k] = (c0, c1) + KeySwitch(c2)      -- keyswitch.hip's launch_key_switch over the chain's K ciphertexts
//
// Relinearization is linear, so this decrypts to what sum_c EvalMult(w_c, u_{c,k}) decrypts to, at K key
// switches instead of C K.  Sums mod q_t are exact: out[k] is, bit for bit, dot.hip's result on the stacked
// weights against the stacked k-th column, and at C = 1 keyswitch.hip's EvalMult.
//
//   wsum_tensor_intt_kernel  ks_tensor_intt_kernel's place in the chain and its geometry, the one product of
//                            each term replaced by the sum over the learner axis
//   launch_key_switch        keyswitch.hip's, unchanged
//
// The updates may sit at a higher level than the weights (Lu >= Ll): the first Ll towers of each update
// polynomial are read in place at polynomial stride Lu N; towers [Ll, Lu) are never touched.
#include <hip/hip_runtime.h>

#include "dot_dev.h"
#include "shelfi_internal.h"

namespace shelfi {

// No mid-run fold.  An accumulator starts at 0 and takes, in c1, two products of canonical residues a learner,
// each <= (q - 1)^2: the run of dot_dev.h's fold-interval bound with G = C ciphertexts.  dot_fold_interval(q) is
// at least 128 for every tower the library builds (b <= 60 bits: 2 * 128 (2^60 - 1)^2 < 2^128), so C learners
// never wrap an accumulator while C <= 128; at the cap of 32 c1 holds at most 64 products < 2^120, a sum below
// 2^126.  One dot_red128 (any 128-bit value -> [0, q)) per accumulator at the end is therefore exact.
static_assert(kWsumMaxLearners <= 128, "wsum_tensor_intt_kernel folds its accumulators once, at the end: the learner "
                                       "cap must stay within dot_fold_interval's smallest value (60-bit towers)");

// By value in the kernel arguments (2 x 32 base pointers: 512 bytes), as gram.hip's GramArgs.  u[c] is learner
// c's first update ciphertext of the chain, w[c] its weight for that ciphertext.
struct WsumArgs {
  const uint64_t* u[kWsumMaxLearners];
  const uint64_t* w[kWsumMaxLearners];
};

// PERK: a weight ciphertext per update ciphertext -- the weights are read once, like the updates, with
// ld_pair's non-temporal loads.  Otherwise learner c's one weight is re-read by every k: plain cached loads.
template <bool PERK>
__device__ __forceinline__ ulonglong2 wsum_ld_weight(const uint64_t* p) {
  if (PERK) return ld_pair(p);
  return *reinterpret_cast<const ulonglong2*>(p);
}

// One workgroup per (k, tower, NTT block), 256 threads, 16-byte pairs: ks_tensor_intt_kernel's geometry, but k
// varies FASTEST in blockIdx.x, so that the workgroups in flight together share a (tower, block) and -- with
// one weight a learner -- the same C x 2 x block bytes of weights (1 MiB at C = 32 and 2^11-word blocks), which
// then come from L2.  A thread walks its pairs one after another (a pair's six 128-bit accumulators are 24
// registers; holding a 2^11 block's four pairs together would take 96 for them alone and cost the waves that
// hide the loads' latency); within a pair U = 2 learners' 8 loads are issued before any is used, as
// dot_partial_kernel's.  c0, c1 -> out, c2 -> d2e and, through the first inverse stages in LDS, d2c.
template <bool PERK>
__global__ __launch_bounds__(256) void wsum_tensor_intt_kernel(const WsumArgs g, uint32_t C, uint32_t K, uint32_t Lu,
                                                               uint32_t Ll, uint32_t logN, uint32_t blkLog,
                                                               const uint64_t* __restrict__ itw,
                                                               const uint64_t* __restrict__ itwp,
                                                               const TowerConst* __restrict__ tq,
                                                               uint64_t* __restrict__ out,
                                                               uint64_t* __restrict__ d2e,
                                                               uint64_t* __restrict__ d2c) {
  extern __shared__ __attribute__((aligned(16))) uint64_t sm[];
  constexpr int U = 2;
  const uint32_t N = 1u << logN, blk = 1u << blkLog, sh = logN - blkLog;
  const uint64_t k = blockIdx.x % K;
  const uint32_t tb = blockIdx.x / K;  // t * 2^sh + b
  const uint32_t t = tb >> sh, b = tb & ((1u << sh) - 1);
  const TowerConst c = tq[t];
  const uint64_t off = ((uint64_t)t << logN) + ((uint64_t)b << blkLog);
  const uint64_t upoly = (uint64_t)Lu << logN, poly = (uint64_t)Ll << logN;
  const uint64_t iu = k * 2 * upoly + off;                // the update's c0 block; its c1 block upoly words on
  const uint64_t iw = (PERK ? k * 2 * poly : 0) + off;    // the weight's
  const uint64_t io = k * 2 * poly + off;                 // the output's
  const uint64_t id = ((k * Ll + t) << logN) + ((uint64_t)b << blkLog);
  ulonglong2* O0 = reinterpret_cast<ulonglong2*>(out + io);
  ulonglong2* O1 = reinterpret_cast<ulonglong2*>(out + io + poly);
  ulonglong2* E2 = reinterpret_cast<ulonglong2*>(d2e + id);
  for (uint32_t p = threadIdx.x; p < blk / 2; p += 256) {
    du128 c0x = 0, c0y = 0, c1x = 0, c1y = 0, c2x = 0, c2y = 0;
    const auto take = [&](const ulonglong2& w0, const ulonglong2& w1, const ulonglong2& u0, const ulonglong2& u1) {
      c0x += (du128)w0.x * u0.x;
      c0y += (du128)w0.y * u0.y;
      c1x += (du128)w0.x * u1.x;
      c1x += (du128)w1.x * u0.x;
      c1y += (du128)w0.y * u1.y;
      c1y += (du128)w1.y * u0.y;
      c2x += (du128)w1.x * u1.x;
      c2y += (du128)w1.y * u1.y;
    };
    const uint64_t eu = iu + 2u * p, ew = iw + 2u * p;
    uint32_t l = 0;
    for (; l + U <= C; l += U) {
      ulonglong2 w0[U], w1[U], u0[U], u1[U];
#pragma unroll
      for (int v = 0; v < U; ++v) {
        const uint64_t* up = g.u[l + v] + eu;
        const uint64_t* wp = g.w[l + v] + ew;
        u0[v] = ld_pair(up);
        u1[v] = ld_pair(up + upoly);
        w0[v] = wsum_ld_weight<PERK>(wp);
        w1[v] = wsum_ld_weight<PERK>(wp + poly);
      }
#pragma unroll
      for (int v = 0; v < U; ++v) take(w0[v], w1[v], u0[v], u1[v]);
    }
    for (; l < C; ++l) {
      const uint64_t* up = g.u[l] + eu;
      const uint64_t* wp = g.w[l] + ew;
      const ulonglong2 u0 = ld_pair(up), u1 = ld_pair(up + upoly);
      take(wsum_ld_weight<PERK>(wp), wsum_ld_weight<PERK>(wp + poly), u0, u1);
    }
    const ulonglong2 r0 = make_ulonglong2(dot_red128(c0x, c), dot_red128(c0y, c));
    const ulonglong2 r1 = make_ulonglong2(dot_red128(c1x, c), dot_red128(c1y, c));
    const ulonglong2 r2 = make_ulonglong2(dot_red128(c2x, c), dot_red128(c2y, c));
    O0[p] = r0;
    O1[p] = r1;
    E2[p] = r2;
    lds_put2(sm, p, r2);
  }
  __syncthreads();
  ks_intt_block_out(sm, blkLog, b, logN, itw + (uint64_t)t * N, itwp + (uint64_t)t * N, c, d2c + id);
}

void launch_wsum(const KsArgs& a, const DeviceTables& dtq, const DeviceTables& dte, const DeviceTables* dtf,
                 const uint64_t* evk, const uint64_t* evk_sh, const uint64_t* const* u, uint32_t Lu,
                 const uint64_t* const* w, bool per_k, uint32_t C, uint64_t k0, uint64_t kc, uint64_t* out,
                 void* scratch, hipStream_t s) {
  if (!kc) return;
  if (C < 1 || C > (uint32_t)kWsumMaxLearners || Lu < a.Ll) throw Error{SHELFI_ERR_ARG, "EvalLinearWSum: bad learner count or level"};
  const uint32_t blkLog = ntt_block_log(a.logN), sh = a.logN - blkLog;
  const uint64_t blocks = (kc * a.Ll) << sh;
  if (blocks > 0x7FFFFFFFull) throw Error{SHELFI_ERR_ARG, "EvalLinearWSum batch too large"};
  const uint64_t uctw = 2ull * Lu << a.logN, ctw = 2ull * a.Ll << a.logN;
  WsumArgs g{};
  for (uint32_t i = 0; i < C; ++i) {
    g.u[i] = u[i] + k0 * uctw;
    g.w[i] = w[i] + (per_k ? k0 * ctw : 0);
  }
  const KsScratch ks = ks_scratch_layout(a, kc, scratch);
  uint64_t* o = out + k0 * ctw;
  const auto front = per_k ? wsum_tensor_intt_kernel<true> : wsum_tensor_intt_kernel<false>;
  hipLaunchKernelGGL(front, dim3((uint32_t)blocks), dim3(256), sizeof(uint64_t) << blkLog, s, g, C, (uint32_t)kc, Lu,
                     a.Ll, a.logN, blkLog, dtq.ipsi_rev, dtq.ipsi_rev_sh, a.tq, o, ks.d2e, ks.d2c);
  SHELFI_HIP(hipGetLastError());
  launch_key_switch(a, dtq, dte, dtf, evk, evk_sh, kc, o, scratch, s);
}

}  // namespace shelfi
