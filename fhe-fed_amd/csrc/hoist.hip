// hoist.hip — hoisted rotations on gfx950: R rotations of one ciphertext from ONE digit
// decomposition (PALISADE's EvalFastRotationPrecompute / EvalFastRotation).
//
//   decompose once   D_j = digit j of c1 over Q_l u P in EVALUATION: the digit's own towers are c1's
//                    residues, its foreign towers NTT(ModUp_j(INTT(c1))) -- keyswitch.hip's arithmetic
//   per rotation r   U_r = sum_j sigma_{g_r}(D_j) (.) (b_{r,j}, a_{r,j})      over Q_l u P
//                    out_r = (sigma_{g_r}(c0), 0) + ModDown(U_r)
//
// Everything in front of the inner product is the input's alone, so it runs once: the front pass (c1 to
// d2e and through its first INTT stages, no gather), the INTT columns and ModUp (launch_ks_modup).  The
// automorphism moves to the one place where every digit's block already sits in EVALUATION form in LDS:
// sigma_g maps an NTT block onto an NTT block (galois_src, dev_common.h), so a workgroup that owns a SOURCE
// block (ct, tower, b') runs the foreign digits' last NTT stages once, with block b' twiddles, and then for
// every rotation of its group gathers the output block whose sources are b' out of LDS, multiplies by that
// rotation's key at the output positions and writes that rotation's accumulators.  ModDown and the finish
// are keyswitch.hip's, batched over the group's accumulators.
//
// Not bit-equal to launch_rotate, which decomposes sigma_g(c1): the approximate basis conversion does not
// commute with the sign flips of sigma_g.  Both are valid rotations (§2.21).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dev_common.h"
#include "shelfi_internal.h"

namespace shelfi {

// ------------------------------------------------------------- front pass ----
// One workgroup per (ct, tower, block): c1's block to d2e (EVALUATION, the digits' own towers) and through
// the first inverse stages in LDS to d2c.  rot_gather_intt_kernel without the gather and without `out`.
__global__ __launch_bounds__(256) void hoist_front_kernel(const uint64_t* __restrict__ ct, uint32_t Ll,
                                                          uint32_t logN, uint32_t blkLog,
                                                          const uint64_t* __restrict__ itw,
                                                          const uint64_t* __restrict__ itwp,
                                                          const TowerConst* __restrict__ tq,
                                                          uint64_t* __restrict__ d2e, uint64_t* __restrict__ d2c) {
  extern __shared__ __attribute__((aligned(16))) uint64_t sm[];
  const uint32_t N = 1u << logN, blk = 1u << blkLog, sh = logN - blkLog;
  const uint64_t row = blockIdx.x >> sh;  // k * Ll + t
  const uint32_t b = blockIdx.x & ((1u << sh) - 1);
  const uint64_t k = row / Ll;
  const uint32_t t = (uint32_t)(row % Ll);
  const TowerConst c = tq[t];
  const uint32_t boff = b << blkLog;
  const uint64_t id = (row << logN) + boff;
  const ulonglong2* S1 = reinterpret_cast<const ulonglong2*>(ct + (((k * 2 + 1) * Ll + t) << logN) + boff);
  ulonglong2* E = reinterpret_cast<ulonglong2*>(d2e + id);
  for (uint32_t p = threadIdx.x; p < blk / 2; p += 256) {
    const ulonglong2 v = S1[p];
    E[p] = v;
    lds_put2(sm, p, v);
  }
  __syncthreads();
  ks_intt_block_out(sm, blkLog, b, logN, itw + (uint64_t)t * N, itwp + (uint64_t)t * N, c, d2c + id);
}

// --------------------------------------------------- sigma_g(c0) into out_r ----
// out_r = (sigma_{g_r}(c0), 0) for every rotation of the group (blockIdx.y): one thread per 16-byte pair of
// an output row (k, t), its source pair swapped when the source position is odd (rot_gather_intt_kernel's
// gather).  The finish of the key switch adds into out_r.
__global__ __launch_bounds__(256) void hoist_c0_kernel(const uint64_t* __restrict__ ct, uint32_t Ll, uint32_t logN,
                                                       HoistGroup grp) {
  const HoistRot& h = grp.r[blockIdx.y];
  const uint32_t bpr = 1u << (logN - 9);  // blocks per row: 256 threads x 2 residues
  const uint64_t row = blockIdx.x / bpr;  // k * Ll + t
  const uint64_t k = row / Ll;
  const uint32_t t = (uint32_t)(row % Ll);
  const uint32_t p = (blockIdx.x % bpr) * 256 + threadIdx.x;
  const uint64_t r0 = (k * 2 * Ll + t) << logN, r1 = ((k * 2 + 1) * Ll + t) << logN;
  const uint32_t src = galois_src(2 * p, h.g, logN);
  ulonglong2 v = reinterpret_cast<const ulonglong2*>(ct + r0)[src >> 1];
  if (src & 1) v = make_ulonglong2(v.y, v.x);
  reinterpret_cast<ulonglong2*>(h.out + r0)[p] = v;
  reinterpret_cast<ulonglong2*>(h.out + r1)[p] = make_ulonglong2(0, 0);
}

// --------------------------------- last NTT pass + the hoisted inner products ----
// The products of one rotation: the workgroup's source block b' (every foreign digit's block canonical in
// its LDS slot, slot j at sm + j * slot_words, element i at Idx(i)) gathered into output block b_r, times
// key r, into that rotation's accumulators.  own: the row (k, t) of d2e, for the digits that own tower t.
template <class Idx>
__device__ __forceinline__ void hoist_products(const uint64_t* sm, uint32_t slot_words, Idx idx, const KsArgs& a,
                                               uint32_t blkLog, uint32_t b, uint64_t k, uint64_t K, uint32_t t,
                                               uint32_t own_mask, const uint64_t* __restrict__ own,
                                               const HoistRot& h, uint64_t* __restrict__ accQ,
                                               uint64_t* __restrict__ accP) {
  const uint32_t blk = 1u << blkLog;
  const uint64_t q = a.te[t].q;
  const uint32_t TF = a.Lfull + a.kP;
  const uint32_t tk = t < a.Ll ? t : a.Lfull + (t - a.Ll);  // the key's tower
  // the output block whose sources are block b: sigma's inverse is sigma of g^-1
  const uint32_t br = galois_src(b << blkLog, h.ginv, a.logN) >> blkLog;
  const uint32_t boff = br << blkLog;
  ulonglong2 *o0, *o1;
  if (t < a.Ll) {
    o0 = reinterpret_cast<ulonglong2*>(accQ + ((((k * 2 + 0) * a.Ll + t)) << a.logN) + boff);
    o1 = reinterpret_cast<ulonglong2*>(accQ + ((((k * 2 + 1) * a.Ll + t)) << a.logN) + boff);
  } else {
    const uint32_t m = t - a.Ll;
    o0 = reinterpret_cast<ulonglong2*>(accP + ((((k * 2 + 0) * a.kP + m)) << a.logN) + boff);
    o1 = reinterpret_cast<ulonglong2*>(accP + ((((k * 2 + 1) * a.kP + m)) << a.logN) + boff);
  }
  const ulonglong2* own2 = reinterpret_cast<const ulonglong2*>(own);
  for (uint32_t p = threadIdx.x; p < blk / 2; p += 256) {
    const uint32_t src = galois_src(boff + 2 * p, h.g, a.logN);  // in block b; its pair is src ^ 1
    const uint32_t loc = src & (blk - 1) & ~1u;
    const bool odd = src & 1;
    ulonglong2 u0 = make_ulonglong2(0, 0), u1 = make_ulonglong2(0, 0);
    for (uint32_t j = 0; j < a.dn; ++j) {
      ulonglong2 v = (own_mask & (1u << j))
                         ? own2[src >> 1]
                         : *reinterpret_cast<const ulonglong2*>(sm + (uint64_t)j * slot_words + idx(loc));
      if (odd) v = make_ulonglong2(v.y, v.x);
      const uint64_t kb = ((((uint64_t)j * TF + tk)) << a.logN) + boff + 2ull * p;
      const uint64_t ka = ((((uint64_t)(a.dnFull + j) * TF + tk)) << a.logN) + boff + 2ull * p;
      const ulonglong2 bv = *reinterpret_cast<const ulonglong2*>(h.key + kb);
      const ulonglong2 bs = *reinterpret_cast<const ulonglong2*>(h.key_sh + kb);
      const ulonglong2 av = *reinterpret_cast<const ulonglong2*>(h.key + ka);
      const ulonglong2 as = *reinterpret_cast<const ulonglong2*>(h.key_sh + ka);
      u0.x = addmod(u0.x, shoup_mul(v.x, bv.x, bs.x, q), q);
      u0.y = addmod(u0.y, shoup_mul(v.y, bv.y, bs.y, q), q);
      u1.x = addmod(u1.x, shoup_mul(v.x, av.x, as.x, q), q);
      u1.y = addmod(u1.y, shoup_mul(v.y, av.y, as.y, q), q);
    }
    o0[p] = u0;
    o1[p] = u1;
  }
}

// One workgroup per (ct, tower t of Q_l u P, SOURCE block b') and slice blockIdx.y of the group's rotations
// (`per` rotations a slice): ks_inner_blocks_kernel's load and last NTT stages, once, then canonical residues
// in LDS and hoist_products per rotation.  accQ [n][K][2][Ll][N], accP [n][K][2][kP][N] for the group's n.
__global__ __launch_bounds__(256) void hoist_inner_blocks_kernel(const uint64_t* __restrict__ d2e,
                                                                 const uint64_t* __restrict__ ext, uint64_t K,
                                                                 KsArgs a, uint32_t blkLog,
                                                                 const uint64_t* __restrict__ tw,
                                                                 const uint64_t* __restrict__ twp, HoistGroup grp,
                                                                 uint32_t per, uint64_t* __restrict__ accQ,
                                                                 uint64_t* __restrict__ accP) {
  extern __shared__ __attribute__((aligned(16))) uint64_t sm[];
  const uint32_t N = 1u << a.logN, blk = 1u << blkLog, sh = a.logN - blkLog;
  const uint64_t row = blockIdx.x >> sh;  // k * T + t
  const uint32_t b = blockIdx.x & ((1u << sh) - 1);
  const uint64_t k = row / a.T;
  const uint32_t t = (uint32_t)(row % a.T);
  const uint64_t q = a.te[t].q;
  const uint64_t boff = (uint64_t)b << blkLog;
  uint32_t own_mask = 0;
  for (uint32_t j = 0; j < a.dn; ++j) {
    uint32_t s, cnt;
    digit_span(a, j, s, cnt);
    if (t >= s && t < s + cnt) {
      own_mask |= 1u << j;
      continue;
    }
    const uint32_t u = t < s ? t : t - cnt;
    const ulonglong2* src = reinterpret_cast<const ulonglong2*>(
        ext + ext_base(a, j, K) + ((k * (a.T - cnt) + u) << a.logN) + boff);
    for (uint32_t p = threadIdx.x; p < blk / 2; p += 256) lds_put2(sm + ((uint64_t)j << blkLog), p, src[p]);
  }
  __syncthreads();
  for (uint32_t j = 0; j < a.dn; ++j)
    if (!(own_mask & (1u << j))) {
      uint64_t* slot = sm + ((uint64_t)j << blkLog);
      ntt_fwd_block_stages(slot, blkLog, b, a.logN, tw + (uint64_t)t * N, twp + (uint64_t)t * N, q);
      // canonical once, not once per rotation (each thread its own pairs; the barrier below publishes them)
      for (uint32_t p = threadIdx.x; p < blk / 2; p += 256) {
        const ulonglong2 v = lds_get2(slot, p);
        lds_put2(slot, p, make_ulonglong2(canon8(v.x, q), canon8(v.y, q)));
      }
    }
  __syncthreads();
  const uint64_t* own = d2e + ((k * a.Ll + t) << a.logN);
  const uint64_t KN = K << a.logN;
  const uint32_t r1 = min(grp.n, (blockIdx.y + 1) * per);
  for (uint32_t r = blockIdx.y * per; r < r1; ++r)
    hoist_products(sm, blk, [](uint32_t i) { return lds_sw(i); }, a, blkLog, b, k, K, t, own_mask, own, grp.r[r],
                   accQ + (uint64_t)r * KN * 2 * a.Ll, accP + (uint64_t)r * KN * 2 * a.kP);
}

// The same at compile-time shape (ks_inner_blocks_ct's load: fwd_block_pass_ct over the per-block twiddle
// slices of block b', canonical residues in padded LDS slots of lpad_size(BL) u64); the gather reads the
// padded slots through lpad, as the stages wrote them.
template <int BL, int K1, int K2, int K3, int K4>
__global__ __launch_bounds__(256) void hoist_inner_blocks_ct(const uint64_t* __restrict__ d2e,
                                                             const uint64_t* __restrict__ ext, uint64_t K,
                                                             KsArgs a, const ulonglong2* __restrict__ twb,
                                                             HoistGroup grp, uint32_t per,
                                                             uint64_t* __restrict__ accQ,
                                                             uint64_t* __restrict__ accP) {
  extern __shared__ __attribute__((aligned(16))) uint64_t sm[];
  constexpr uint32_t SL = lpad_size(BL);
  const uint32_t sh = a.logN - BL;
  const uint64_t row = blockIdx.x >> sh;  // k * T + t
  const uint32_t b = blockIdx.x & ((1u << sh) - 1);
  const uint64_t k = row / a.T;
  const uint32_t t = (uint32_t)(row % a.T);
  const TowerConst& c = a.te[t];
  const uint64_t q = c.q;
  const uint64_t boff = (uint64_t)b << BL;
  const ulonglong2* __restrict__ tb = twb + ((uint64_t)t << a.logN) + boff;
  uint32_t own_mask = 0;
  for (uint32_t j = 0; j < a.dn; ++j) {
    uint32_t s, cnt;
    digit_span(a, j, s, cnt);
    if (t >= s && t < s + cnt) {
      own_mask |= 1u << j;
      continue;
    }
    const uint32_t u = t < s ? t : t - cnt;
    uint64_t* slot = sm + (uint64_t)j * SL;
    fwd_block_pass_ct<BL, K1, K2, K3, K4>(ext + ext_base(a, j, K) + ((k * (a.T - cnt) + u) << a.logN) + boff,
                                          tb, q, c.n8q, slot, [&](uint32_t j0, auto& x) {
                                            const uint32_t pj0 = lpad(j0);
#pragma unroll
                                            for (int m = 0; m < (1 << K4); ++m) slot[pj0 + m] = red_any(x[m], c);
                                          });
  }
  __syncthreads();
  const uint64_t* own = d2e + ((k * a.Ll + t) << a.logN);
  const uint64_t KN = K << a.logN;
  const uint32_t r1 = min(grp.n, (blockIdx.y + 1) * per);
  for (uint32_t r = blockIdx.y * per; r < r1; ++r)
    hoist_products(sm, SL, [](uint32_t i) { return lpad(i); }, a, (uint32_t)BL, b, k, K, t, own_mask, own, grp.r[r],
                   accQ + (uint64_t)r * KN * 2 * a.Ll, accP + (uint64_t)r * KN * 2 * a.kP);
}

static dim3 hoist_grid(uint64_t rows, uint32_t per_row, uint32_t y = 1) {
  const uint64_t b = rows * per_row;
  if (b > 0x7FFFFFFFull) throw Error{SHELFI_ERR_ARG, "rotation batch too large"};
  return dim3((uint32_t)b, y);
}

// d2e | d2c | ext of K ciphertexts: the decomposition every rotation shares
size_t hoist_shared_bytes(const KsArgs& a, uint64_t K) {
  return ((K << a.logN) * 8 * (2ull * a.Ll + ks_ext_towers(a.Ll, a.kP, a.dn, a.alpha)) + 63) & ~(size_t)63;
}
// accQ | accP | z of K ciphertexts: one rotation in flight
size_t hoist_acc_bytes(const KsArgs& a, uint64_t K) {
  return (K << a.logN) * 8 * (2ull * a.Ll + 2ull * a.kP + 2ull * a.Ll);
}

void launch_hoist_decompose(const KsArgs& a, const DeviceTables& dtq, const DeviceTables& dte,
                            const DeviceTables* dtf, const uint64_t* ct, uint64_t K, void* scratch, hipStream_t s) {
  if (!K) return;
  const uint32_t blkLog = ntt_block_log(a.logN), sh = a.logN - blkLog;
  const uint64_t KN = K << a.logN;
  uint64_t* d2e = reinterpret_cast<uint64_t*>(scratch);
  uint64_t *d2c = d2e + KN * a.Ll, *ext = d2c + KN * a.Ll;
  hipLaunchKernelGGL(hoist_front_kernel, hoist_grid(K * a.Ll, 1u << sh), dim3(256), sizeof(uint64_t) << blkLog, s, ct,
                     a.Ll, a.logN, blkLog, dtq.ipsi_rev, dtq.ipsi_rev_sh, a.tq, d2e, d2c);
  SHELFI_HIP(hipGetLastError());
  launch_ks_modup(a, dtq, dte, dtf, K, d2c, ext, s);
}

void launch_hoist_rotations(const KsArgs& a, const DeviceTables& dtq, const DeviceTables& dte, const HoistGroup& grp,
                            bool out_contiguous, const uint64_t* ct, uint64_t K, void* scratch, hipStream_t s) {
  if (!K || !grp.n) return;
  if (a.logN < 9) throw Error{SHELFI_ERR_ARG, "rotation: unsupported ring dimension"};
  const uint32_t blkLog = ntt_block_log(a.logN), sh = a.logN - blkLog, nb = 1u << sh, n = grp.n;
  const uint64_t KN = K << a.logN;
  const uint64_t* d2e = reinterpret_cast<const uint64_t*>(scratch);
  const uint64_t* ext = d2e + 2 * KN * a.Ll;
  uint64_t* accQ = reinterpret_cast<uint64_t*>(static_cast<char*>(scratch) + hoist_shared_bytes(a, K));
  uint64_t* accP = accQ + (uint64_t)n * KN * 2 * a.Ll;
  uint64_t* z = accP + (uint64_t)n * KN * 2 * a.kP;
  hipLaunchKernelGGL(hoist_c0_kernel, hoist_grid(K * a.Ll, 1u << (a.logN - 9), n), dim3(256), 0, s, ct, a.Ll, a.logN,
                     grp);
  SHELFI_HIP(hipGetLastError());
  // rotations one workgroup serves behind its one NTT pass (SHELFI_HOIST_KEYS_PER_PASS: A/B runs)
  const uint32_t want = switches().hoist_keys ? (uint32_t)switches().hoist_keys : (uint32_t)kHoistKeysPerPass;
  const uint32_t per = std::min(want, n), slices = (n + per - 1) / per;
  if (sh > 0 && blkLog == 11 && dte.red_ok) {
    hipLaunchKernelGGL((hoist_inner_blocks_ct<11, 3, 3, 3, 2>), hoist_grid(K * a.T, nb, slices), dim3(256),
                       sizeof(uint64_t) * lpad_size(11) * a.dn, s, d2e, ext, K, a, dte.tw_fwd_blk, grp, per, accQ,
                       accP);
  } else {
    const size_t lds = (sizeof(uint64_t) << blkLog) * a.dn;
    if (lds > 65536)
      SHELFI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&hoist_inner_blocks_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(hoist_inner_blocks_kernel, hoist_grid(K * a.T, nb, slices), dim3(256), lds, s, d2e, ext, K, a,
                       blkLog, dte.psi_rev, dte.psi_rev_sh, grp, per, accQ, accP);
  }
  SHELFI_HIP(hipGetLastError());
  // ModDown over the group's n K accumulators in one batch; the finish too where the outputs are one batch
  launch_ks_moddown(a, dtq, dte, (uint64_t)n * K, accP, z, s);
  if (out_contiguous) {
    launch_ks_finish(a, dtq, (uint64_t)n * K, z, accQ, grp.r[0].out, s);
  } else {
    for (uint32_t r = 0; r < n; ++r)
      launch_ks_finish(a, dtq, K, z + (uint64_t)r * KN * 2 * a.Ll, accQ + (uint64_t)r * KN * 2 * a.Ll, grp.r[r].out, s);
  }
}

}  // namespace shelfi
