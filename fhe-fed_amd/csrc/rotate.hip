// rotate.hip — slot rotations on gfx950: EvalAtIndex (the reference's mkhe.cpp:124
// EvalAtIndexKeyGen, :274 EvalSumKeyGen, :372 EvalSum) as the automorphism sigma_g: X -> X^g
// followed by keyswitch.hip's HYBRID key switch, and the plain ciphertext add EvalSum needs.
//
//   Rotate(ct, r)   g = 5^r mod 2N (r < 0: the inverse);  (c0, c1) -> (sigma_g(c0) + u0, u1),
//                   (u0, u1) = KeySwitch(sigma_g(c1)) under the key sigma_g(s) -> s
//   sigma_g         in EVALUATION, in the NTT's bit-reversed order, a permutation of positions:
//                   out[j] = in[galois_src(j)] (dev_common.h) -- no arithmetic, no table
//
// The front pass gathers on load: a workgroup owns one output block (ct, tower, block) and reads
// its sources.  It must own whole output blocks, because the block of sigma_g(c1) goes through the
// first inverse-NTT stages in LDS exactly as the tensor pass's c2 does; a scatter on store would
// spread one workgroup's elements over blocks other workgroups transform.  The gather is local:
// sigma_g maps every aligned run of 2^k positions onto an aligned run of 2^k positions (the low
// k bits of a position are the top k bits of its exponent), so pairs (2p, 2p + 1) come from one
// aligned 16-byte word, possibly swapped, a wave's 1 KiB of output reads exactly 1 KiB of input,
// and a block reads exactly one block: every fetched line is used in full, once.
//
// The finish of the key switch adds into `out`, so the front pass writes sigma_g(c0) to out's
// first component and zeros to its second; everything behind it is launch_key_switch.
#include <hip/hip_runtime.h>

#include "dev_common.h"
#include "shelfi_internal.h"

namespace shelfi {

// One workgroup per (ct, tower, block); ct and out must not overlap (the gather reads the row).
__global__ __launch_bounds__(256) void rot_gather_intt_kernel(const uint64_t* __restrict__ ct, uint32_t Ll,
                                                              uint32_t logN, uint32_t blkLog, uint32_t g,
                                                              const uint64_t* __restrict__ itw,
                                                              const uint64_t* __restrict__ itwp,
                                                              const TowerConst* __restrict__ tq,
                                                              uint64_t* __restrict__ out,
                                                              uint64_t* __restrict__ d2e,
                                                              uint64_t* __restrict__ d2c) {
  extern __shared__ __attribute__((aligned(16))) uint64_t sm[];
  const uint32_t N = 1u << logN, blk = 1u << blkLog, sh = logN - blkLog;
  const uint64_t row = blockIdx.x >> sh;  // k * Ll + t
  const uint32_t b = blockIdx.x & ((1u << sh) - 1);
  const uint64_t k = row / Ll;
  const uint32_t t = (uint32_t)(row % Ll);
  const TowerConst c = tq[t];
  const uint64_t r0 = (k * 2 * Ll + t) << logN, r1 = ((k * 2 + 1) * Ll + t) << logN;  // rows of c0, c1
  const uint32_t boff = b << blkLog;
  const uint64_t id = (row << logN) + boff;
  const ulonglong2* S0 = reinterpret_cast<const ulonglong2*>(ct + r0);
  const ulonglong2* S1 = reinterpret_cast<const ulonglong2*>(ct + r1);
  ulonglong2* O0 = reinterpret_cast<ulonglong2*>(out + r0 + boff);
  ulonglong2* O1 = reinterpret_cast<ulonglong2*>(out + r1 + boff);
  ulonglong2* E = reinterpret_cast<ulonglong2*>(d2e + id);
  for (uint32_t p = threadIdx.x; p < blk / 2; p += 256) {
    const uint32_t src = galois_src(boff + 2 * p, g, logN);  // < N; its pair is src ^ 1
    ulonglong2 v0 = S0[src >> 1], v1 = S1[src >> 1];
    if (src & 1) {
      v0 = make_ulonglong2(v0.y, v0.x);
      v1 = make_ulonglong2(v1.y, v1.x);
    }
    O0[p] = v0;
    O1[p] = make_ulonglong2(0, 0);
    E[p] = v1;
    lds_put2(sm, p, v1);
  }
  __syncthreads();
  ks_intt_block_out(sm, blkLog, b, logN, itw + (uint64_t)t * N, itwp + (uint64_t)t * N, c, d2c + id);
}

void launch_rotate(const KsArgs& a, const DeviceTables& dtq, const DeviceTables& dte, const DeviceTables* dtf,
                   const uint64_t* rk, const uint64_t* rk_sh, uint32_t g, const uint64_t* ct, uint64_t K,
                   uint64_t* out, void* scratch, hipStream_t s) {
  if (!K) return;
  const uint32_t blkLog = ntt_block_log(a.logN), sh = a.logN - blkLog;
  const KsScratch ks = ks_scratch_layout(a, K, scratch);
  const uint64_t blocks = (K * a.Ll) << sh;
  if (blocks > 0x7FFFFFFFull) throw Error{SHELFI_ERR_ARG, "rotation batch too large"};
  hipLaunchKernelGGL(rot_gather_intt_kernel, dim3((uint32_t)blocks), dim3(256), sizeof(uint64_t) << blkLog, s, ct,
                     a.Ll, a.logN, blkLog, g, dtq.ipsi_rev, dtq.ipsi_rev_sh, a.tq, out, ks.d2e, ks.d2c);
  SHELFI_HIP(hipGetLastError());
  launch_key_switch(a, dtq, dte, dtf, rk, rk_sh, K, out, scratch, s);
}

// out = a + b mod q_t: one thread per residue pair, rows tower-uniform (row = (k * 2 + poly) * Ll + t).
// out may be a or b: each thread reads its pair before writing it.
__global__ __launch_bounds__(256) void ct_add_kernel(const uint64_t* a, const uint64_t* b, uint32_t Ll,
                                                     uint32_t logN, const TowerConst* __restrict__ tq,
                                                     uint64_t* out) {
  const uint32_t bpr = 1u << (logN - 9);  // blocks per row: 256 threads x 2 residues
  const uint64_t row = blockIdx.x / bpr;
  const uint64_t q = tq[row % Ll].q;
  const uint64_t i = (row << (logN - 1)) + (uint64_t)(blockIdx.x % bpr) * 256 + threadIdx.x;
  const ulonglong2 x = reinterpret_cast<const ulonglong2*>(a)[i], y = reinterpret_cast<const ulonglong2*>(b)[i];
  reinterpret_cast<ulonglong2*>(out)[i] = make_ulonglong2(addmod(x.x, y.x, q), addmod(x.y, y.y, q));
}

void launch_ct_add(const uint64_t* a, const uint64_t* b, uint64_t rows, uint32_t Ll, uint32_t logN,
                   const TowerConst* tq, uint64_t* out, hipStream_t s) {
  if (!rows) return;
  const uint64_t blocks = logN < 9 ? ~0ull : rows << (logN - 9);
  if (blocks > 0x7FFFFFFFull) throw Error{SHELFI_ERR_ARG, "ciphertext add: unsupported shape"};
  hipLaunchKernelGGL(ct_add_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, a, b, Ll, logN, tq, out);
  SHELFI_HIP(hipGetLastError());
}

}  // namespace shelfi
