// plain.hip — plaintext operands: the encode without the encrypt, and the pointwise ciphertext /
// plaintext calls.
//
// Kernels:
//   plain_cols         encode's rounding (encrypt's exact arithmetic, enc_cols_fused phase 2 without the
//                      sampler) on register columns, then per tower the signed reduction and the first
//                      NTT stages, stored lazily (< 8q) into the plaintext's own towers
//   plain_blocks_ct    the LDS block stages at compile-time shape, in place, canonical store
//   plain_blocks       the same at run-time shape (towers below 2^40, other block sizes); on rings of
//                      one NTT block it rounds straight into LDS and there is no columns pass
//   plain_op_kernel    cc->EvalMult / EvalAdd / EvalSub(ct, pt): one launch over K x towers x N
//   ct_sub_kernel, ct_neg_kernel    cc->EvalSub(ct, ct), cc->EvalNegate(ct)
// One polynomial per plaintext: a third of encrypt's transform work, none of its ChaCha20 work, no
// public key, and no pbuf -- the scratch is the FFT buffer alone.
#include <hip/hip_runtime.h>

#include <cmath>

#include "dev_common.h"
#include "shelfi_internal.h"
#include "transform_dev.h"

namespace shelfi {

constexpr double kPlainLim = 2305843009213693952.0;  // 2^61: the whole supported range of |m|

// m = round_half_away(fl(fl(v / S) scale)) for the real and the imaginary part of one FFTSpecialInv
// output (1 / S is a power of two: the product is the quotient exactly); GenFlag word 0 for a finite
// |value| above 2^61, word 1 for a non-finite one (enc_range_flag's words)
__device__ __forceinline__ void plain_round(double2 cv, double invS, double scale, GenFlag flag, int64_t& mre,
                                            int64_t& mim) {
  const double vr = __dmul_rn(__dmul_rn(cv.x, invS), scale);
  const double vi = __dmul_rn(__dmul_rn(cv.y, invS), scale);
  if (!(fabs(vr) <= kPlainLim) || !(fabs(vi) <= kPlainLim)) {
    gen_flag_set(flag, 0);
    if (!isfinite(vr) || !isfinite(vi)) gen_flag_set(flag, 1);
  }
  mre = round_half_away(vr);
  mim = round_half_away(vi);
}

// The columns pass: thread = column c of plaintext k, coefficients j = c + BLK r (r < R = 2^LOGR); rows
// r and r + R/2 are the real and imaginary parts of one slot (BLK R/2 = N/2).  The R rounded
// coefficients stay in registers across the tower loop (one polynomial: 2 R VGPRs, where encrypt's
// three could not afford them); per tower the column-stage twiddles psi_rev[1 .. R) are staged in LDS
// as {w, w'} pairs (enc_cols_fused's TWL).  Towers with q >= 2^40 take encrypt's entry: rows >= R/2 go
// into the first stage as u = m + floor(2^62 / q) q, which only its lazy Shoup product reads.
template <int LOGR>
__global__ __launch_bounds__(256) void plain_cols(const double2* __restrict__ fbuf, uint64_t K, uint32_t logN,
                                                  uint32_t logS, uint32_t towers, double scale,
                                                  const TowerConst* __restrict__ tcs,
                                                  const uint64_t* __restrict__ tw,
                                                  const uint64_t* __restrict__ twp, uint64_t* __restrict__ out,
                                                  GenFlag flag) {
  constexpr int R = 1 << LOGR;
  __shared__ ulonglong2 twl[R];
  const uint32_t BLK = (1u << logN) >> LOGR, bpp = BLK / 256;
  const uint64_t k = blockIdx.x / bpp;
  if (k >= K) return;  // workgroup-uniform
  const uint32_t c = (blockIdx.x % bpp) * 256 + threadIdx.x;
  const uint32_t S = 1u << logS, gapLog = logN - 1 - logS;
  const double invS = 1.0 / (double)S;
  int64_t me[R];
#pragma unroll
  for (int r = 0; r < R / 2; ++r) {
    const uint32_t jj = c + BLK * r;  // < N/2
    int64_t mre = 0, mim = 0;
    if ((jj & ((1u << gapLog) - 1)) == 0)
      plain_round(fbuf[k * S + bitrev_dev(jj >> gapLog, logS)], invS, scale, flag, mre, mim);
    me[r] = mre;
    me[r + R / 2] = mim;
  }
  uint64_t* __restrict__ o = out + k * ((uint64_t)towers << logN) + c;
#pragma unroll 1
  for (uint32_t t = 0; t < towers; ++t) {
    __syncthreads();  // the previous tower's twiddle reads are done
    if (threadIdx.x < (uint32_t)R)
      twl[threadIdx.x] = make_ulonglong2(tw[((uint64_t)t << logN) + threadIdx.x], twp[((uint64_t)t << logN) + threadIdx.x]);
    __syncthreads();
    const TowerConst cst = tcs[t];
    const uint64_t q = cst.q;
    uint64_t x[R];
    if (cst.red_ok) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const uint64_t u = (uint64_t)me[r] + cst.bq62;
        x[r] = r < R / 2 ? red_any(u, cst) : u;
      }
    } else {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        x[r] = mod_signed_dev(me[r], cst);
        if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // bound reductions in flight
      }
    }
#pragma unroll
    for (int s = 0; s < LOGR; ++s) {
      const int m = 1 << s, tr = R >> (s + 1);
#pragma unroll
      for (int i = 0; i < m; ++i) {
        const ulonglong2 W = twl[m + i];
#pragma unroll
        for (int jj = 0; jj < tr; ++jj) {
          const int r0 = 2 * i * tr + jj, r1 = r0 + tr;
          if (fwd_red_at(s))
            ct_bfly_s<true>(x[r0], x[r1], W.x, W.y, q, cst.n8q);
          else
            ct_bfly_s<false>(x[r0], x[r1], W.x, W.y, q, cst.n8q);
        }
      }
    }
    // the blocks passes take inputs below 8q
#pragma unroll
    for (int r = 0; r < R; ++r)
      o[((uint64_t)t << logN) + (uint64_t)r * BLK] = fwd_bound(LOGR) > 8 ? csub_neg(x[r], cst.n8q) : x[r];
  }
}

// The blocks pass at compile-time shape (blocks of 2^11 or 2^12 after a columns pass, every q >= 2^40):
// fwd_block_pass_ct in place over tower t's block b of plaintext k -- the first chunk reads the whole
// block into registers before any store -- with the (tower, block) combos dealt per XCD as encrypt's
// block pass deals them, and the canonical residues stored 16 bytes at a time.
template <int BL, int K1, int K2, int K3, int K4>
__global__ __launch_bounds__(256) void plain_blocks_ct(uint64_t* pt, uint32_t towers, uint32_t logN,
                                                       const ulonglong2* __restrict__ twb,
                                                       const TowerConst* __restrict__ tcs, uint32_t xg) {
  __shared__ __attribute__((aligned(16))) uint64_t sm[lpad_size(BL)];
  const uint32_t sh = logN - BL;
  const uint32_t bid = xcd_block(blockIdx.x, xg);
  const uint32_t b = bid & ((1u << sh) - 1);
  const uint32_t poly = bid >> sh, t = poly % towers;
  const TowerConst& c = tcs[t];
  uint64_t* base = pt + ((uint64_t)poly << logN) + ((uint64_t)b << BL);
  fwd_block_pass_ct<BL, K1, K2, K3, K4>(base, twb + ((uint64_t)t << logN) + ((uint64_t)b << BL), c.q, c.n8q, sm,
                                        [&](uint32_t j0, auto& x) {
#pragma unroll
                                          for (int m = 0; m < (1 << K4); m += 2)
                                            *reinterpret_cast<ulonglong2*>(base + j0 + m) =
                                                make_ulonglong2(red_any(x[m], c), red_any(x[m + 1], c));
                                        });
}

// The blocks pass at run-time shape, stages sstart .. logN - 1 in LDS.  sstart = 0 (a ring of one NTT
// block): no columns pass ran; the workgroup rounds its plaintext's coefficients from fbuf itself.
__global__ __launch_bounds__(256) void plain_blocks(uint64_t* __restrict__ pt, const double2* __restrict__ fbuf,
                                                    uint32_t towers, uint32_t logN, uint32_t logS,
                                                    uint32_t sstart, double scale,
                                                    const uint64_t* __restrict__ tw,
                                                    const uint64_t* __restrict__ twp,
                                                    const TowerConst* __restrict__ tcs, GenFlag flag) {
  extern __shared__ __attribute__((aligned(16))) uint64_t sm[];
  const uint32_t blkLog = logN - sstart, blk = 1u << blkLog;
  const uint32_t b = blockIdx.x & ((1u << sstart) - 1);
  const uint64_t poly = blockIdx.x >> sstart;
  const uint32_t t = (uint32_t)(poly % towers);
  const TowerConst& c = tcs[t];
  uint64_t* __restrict__ a = pt + (poly << logN) + ((uint64_t)b << blkLog);
  if (sstart == 0) {
    const uint64_t k = poly / towers;
    const uint32_t S = 1u << logS, gapLog = logN - 1 - logS, half = blk >> 1;
    const double invS = 1.0 / (double)S;
    for (uint32_t jj = threadIdx.x; jj < half; jj += 256) {
      int64_t mre = 0, mim = 0;
      if ((jj & ((1u << gapLog) - 1)) == 0)
        plain_round(fbuf[k * S + bitrev_dev(jj >> gapLog, logS)], invS, scale, flag, mre, mim);
      sm[lds_sw(jj)] = mod_signed_dev(mre, c);
      sm[lds_sw(jj + half)] = mod_signed_dev(mim, c);
    }
  } else {
    for (uint32_t p = threadIdx.x; p < blk / 2; p += 256) lds_put2(sm, p, reinterpret_cast<const ulonglong2*>(a)[p]);
  }
  __syncthreads();
  ntt_fwd_block_stages(sm, blkLog, b, logN, tw + ((uint64_t)t << logN), twp + ((uint64_t)t << logN), c.q);
  for (uint32_t p = threadIdx.x; p < blk / 2; p += 256) {
    const ulonglong2 v = lds_get2(sm, p);
    reinterpret_cast<ulonglong2*>(a)[p] = make_ulonglong2(canon8(v.x, c.q), canon8(v.y, c.q));
  }
}

size_t encode_scratch_bytes(const Params& p, uint64_t K) {  // the FFT buffer [K][S] (complex)
  return K * (uint64_t)p.batch * sizeof(double2) + 64;
}

void launch_encode_plain(const Params& p, const DeviceTables& dt, const double* x, uint64_t n, uint64_t K,
                         uint32_t towers, double scale, uint64_t* pt, void* scratch, GenFlag flag, hipStream_t s) {
  if (!K) return;
  const uint32_t logS = __builtin_ctz(p.batch);
  double2* fbuf = reinterpret_cast<double2*>(scratch);
  launch_encode_fft(p, dt, x, n, K, fbuf, s);
  const uint32_t blkLog = ntt_block_log(p.logN);
  const int logR = (int)(p.logN - blkLog);
  const uint64_t nbCols = K * ((p.N >> logR) / 256), nbBlocks = (K * towers) << logR;
  if (nbBlocks > 0x7FFFFFFFull || nbCols > 0x7FFFFFFFull) throw Error{SHELFI_ERR_ARG, "encode batch too large"};
  if (logR > 0) {
#define PLAIN_COLS(LR)                                                                                          \
  hipLaunchKernelGGL(plain_cols<LR>, dim3((uint32_t)nbCols), dim3(256), 0, s, fbuf, K, p.logN, logS, towers, scale, \
                     dt.tc, dt.psi_rev, dt.psi_rev_sh, pt, flag)
    switch (logR) {
      case 1: PLAIN_COLS(1); break;
      case 2: PLAIN_COLS(2); break;
      case 3: PLAIN_COLS(3); break;
      case 4: PLAIN_COLS(4); break;
      case 5: PLAIN_COLS(5); break;
      case 6: PLAIN_COLS(6); break;
      default: throw Error{SHELFI_ERR_ARG, "unsupported ring dimension"};
    }
#undef PLAIN_COLS
    SHELFI_HIP(hipGetLastError());
  }
  const uint32_t xg = xcd_combos((uint64_t)towers << logR);
  if (logR > 0 && blkLog == 11 && dt.red_ok)
    hipLaunchKernelGGL((plain_blocks_ct<11, 3, 3, 3, 2>), dim3((uint32_t)nbBlocks), dim3(256), 0, s, pt, towers,
                       p.logN, dt.tw_fwd_blk, dt.tc, xg);
  else if (logR > 0 && blkLog == 12 && dt.red_ok)
    hipLaunchKernelGGL((plain_blocks_ct<12, 3, 3, 3, 3>), dim3((uint32_t)nbBlocks), dim3(256), 0, s, pt, towers,
                       p.logN, dt.tw_fwd_blk, dt.tc, xg);
  else
    hipLaunchKernelGGL(plain_blocks, dim3((uint32_t)nbBlocks), dim3(256), sizeof(uint64_t) << blkLog, s, pt, fbuf,
                       towers, p.logN, logS, (uint32_t)logR, scale, dt.psi_rev, dt.psi_rev_sh, dt.tc, flag);
  SHELFI_HIP(hipGetLastError());
}

// ------------------------------------------------------- pointwise calls ----
// a b mod q for canonical a, b below q < 2^60 with no precomputed companion (Barrett): with
// E = bitlength(q) - 1 the product p < 2^(2E+2) gives ph = floor(p / 2^E) < 2^(E+2), and
// k = floor(ph mu / 2^(E+2)), mu = floor(2^(2E+2) / q) (TowerConst::bmu), is floor(p / q) or up to 2
// less; ph is shifted so that the division is the high word of one product.  p - k q < 3q, taken
// mod 2^64 and canonicalised: 2 high and 2 low 64-bit products (mulmod_generic: 3 and 4).
__device__ __forceinline__ uint64_t plain_mulmod(uint64_t a, uint64_t b, const TowerConst& c, uint32_t E) {
  const uint64_t hi = __umul64hi(a, b), lo = a * b;
  const uint64_t ph = (hi << (64 - E)) | (lo >> E);  // 1 <= E <= 59
  const uint64_t k = __umul64hi(ph << (62 - E), c.bmu);
  return canon4(lo - k * c.q, c.q);
}

enum { kPlainMult = 0, kPlainAdd = 1, kPlainSub = 2 };

// One thread = one 16-byte residue pair of tower t of ciphertext k: the plaintext pair is read once and
// applied to c0 and c1 (MULT), or to c0 with c1 copied unless the call is in place (ADD / SUB).
// pstride: words between plaintexts, 0 when one plaintext serves every ciphertext (it stays in L2).
// out may be ct exactly: each thread reads its words before writing them.
template <int OP>
__global__ __launch_bounds__(256) void plain_op_kernel(const uint64_t* ct, const uint64_t* __restrict__ pt,
                                                       uint64_t pstride, uint32_t towers, uint32_t logN,
                                                       const TowerConst* __restrict__ tq, uint64_t* out) {
  const uint32_t bpr = 1u << (logN - 9);  // blocks per row: 256 threads x 2 residues
  const uint64_t row = blockIdx.x / bpr;  // k * towers + t
  const uint64_t k = row / towers;
  const uint32_t t = (uint32_t)(row - k * towers);
  const TowerConst& c = tq[t];
  const uint64_t q = c.q;
  const uint32_t i = (blockIdx.x % bpr) * 256 + threadIdx.x;  // pair index in the row
  const uint64_t TN2 = (uint64_t)towers << (logN - 1);        // pairs per component
  const uint64_t i0 = (k * 2 * towers + t) * (1ull << (logN - 1)) + i, i1 = i0 + TN2;
  const ulonglong2 p = reinterpret_cast<const ulonglong2*>(pt + k * pstride)[((uint64_t)t << (logN - 1)) + i];
  const ulonglong2 x0 = reinterpret_cast<const ulonglong2*>(ct)[i0];
  if (OP == kPlainMult) {
    const ulonglong2 x1 = reinterpret_cast<const ulonglong2*>(ct)[i1];
    const uint32_t E = 63 - (uint32_t)__builtin_clzll(q);  // wave-uniform
    reinterpret_cast<ulonglong2*>(out)[i0] = make_ulonglong2(plain_mulmod(x0.x, p.x, c, E), plain_mulmod(x0.y, p.y, c, E));
    reinterpret_cast<ulonglong2*>(out)[i1] = make_ulonglong2(plain_mulmod(x1.x, p.x, c, E), plain_mulmod(x1.y, p.y, c, E));
  } else {
    reinterpret_cast<ulonglong2*>(out)[i0] =
        OP == kPlainAdd ? make_ulonglong2(addmod(x0.x, p.x, q), addmod(x0.y, p.y, q))
                        : make_ulonglong2(submod(x0.x, p.x, q), submod(x0.y, p.y, q));
    if (out != ct) reinterpret_cast<ulonglong2*>(out)[i1] = reinterpret_cast<const ulonglong2*>(ct)[i1];
  }
}

void launch_plain_op(int op, const uint64_t* ct, const uint64_t* pt, uint64_t K, uint64_t Kp, uint32_t towers,
                     uint32_t logN, const TowerConst* tq, uint64_t* out, hipStream_t s) {
  if (!K) return;
  const uint64_t blocks = logN < 9 ? ~0ull : (K * towers) << (logN - 9);
  if (blocks > 0x7FFFFFFFull) throw Error{SHELFI_ERR_ARG, "plaintext operand: unsupported shape"};
  const uint64_t pstride = Kp == 1 ? 0 : (uint64_t)towers << logN;
#define PLAIN_OP(OP) \
  hipLaunchKernelGGL(plain_op_kernel<OP>, dim3((uint32_t)blocks), dim3(256), 0, s, ct, pt, pstride, towers, logN, tq, out)
  if (op == kPlainMult) PLAIN_OP(kPlainMult);
  else if (op == kPlainAdd) PLAIN_OP(kPlainAdd);
  else PLAIN_OP(kPlainSub);
#undef PLAIN_OP
  SHELFI_HIP(hipGetLastError());
}

// out = a - b mod q_t (b == nullptr: out = -a), rows tower-uniform as in ct_add_kernel; out may be an
// input exactly.  Canonical: a - a = 0 and -0 = 0, never q.
template <bool NEG>
__global__ __launch_bounds__(256) void ct_sub_kernel(const uint64_t* a, const uint64_t* b, uint32_t Ll, uint32_t logN,
                                                     const TowerConst* __restrict__ tq, uint64_t* out) {
  const uint32_t bpr = 1u << (logN - 9);
  const uint64_t row = blockIdx.x / bpr;
  const uint64_t q = tq[row % Ll].q;
  const uint64_t i = (row << (logN - 1)) + (uint64_t)(blockIdx.x % bpr) * 256 + threadIdx.x;
  const ulonglong2 x = reinterpret_cast<const ulonglong2*>(a)[i];
  if (NEG) {
    reinterpret_cast<ulonglong2*>(out)[i] = make_ulonglong2(x.x ? q - x.x : 0, x.y ? q - x.y : 0);
  } else {
    const ulonglong2 y = reinterpret_cast<const ulonglong2*>(b)[i];
    reinterpret_cast<ulonglong2*>(out)[i] = make_ulonglong2(submod(x.x, y.x, q), submod(x.y, y.y, q));
  }
}

void launch_ct_sub(const uint64_t* a, const uint64_t* b, uint64_t rows, uint32_t Ll, uint32_t logN,
                   const TowerConst* tq, uint64_t* out, hipStream_t s) {
  if (!rows) return;
  const uint64_t blocks = logN < 9 ? ~0ull : rows << (logN - 9);
  if (blocks > 0x7FFFFFFFull) throw Error{SHELFI_ERR_ARG, "ciphertext subtract: unsupported shape"};
  if (b)
    hipLaunchKernelGGL(ct_sub_kernel<false>, dim3((uint32_t)blocks), dim3(256), 0, s, a, b, Ll, logN, tq, out);
  else
    hipLaunchKernelGGL(ct_sub_kernel<true>, dim3((uint32_t)blocks), dim3(256), 0, s, a, b, Ll, logN, tq, out);
  SHELFI_HIP(hipGetLastError());
}

}  // namespace shelfi
