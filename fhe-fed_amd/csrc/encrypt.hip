// encrypt.hip — encode + encrypt: FFTSpecialInv, sampling, the forward NTT of v, m + e0, e1 and the
// public-key combine.
//
// Kernels (roofline class in DESIGN.md):
//   fft_inv_*          CKKS special FFT inverse (encode), 2 passes or one workgroup per vector
//   enc_prep_kernel    round/scale the encoded slots + ChaCha20 sampling of (v, e0, e1)
//                      into a compact 10-byte record per coefficient (ckks.cpp:80-81)
//   ntt_fwd_cols_enc   expand the record per tower + first NTT stages
//   enc_cols_fused     both of the above in one kernel, without the record
//   ntt_fwd_blocks_enc(_ct, _pp)  last NTT stages of v, m+e0, e1 + c0 = v*b + (m+e0), c1 = v*a + e1
//                      (_ct: compile-time shape over per-block twiddle slices; _pp: persistent)
//   enc_maxabs_kernel, enc_expand_approx_kernel, enc_combine_kernel  encode's large-value path
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "dev_common.h"
#include "shelfi_internal.h"
#include "transform_dev.h"

namespace shelfi {

// ------------------------------------------------------- special FFT (f64) ----
// FFTSpecialInv (encode): DIF stages len = S..2 with twiddle finv[len/2 + (x mod
// len)], then BitReverse and /S (both folded into enc_prep).  First LOGR stages
// on register columns (reading the learner's real vector directly), the rest in
// LDS blocks of 2^fft_block_log(logS) complex values.
// Slot gi of the call's slot vectors, from its n values.  Real packing: x[gi] + 0i.  Complex packing (CX,
// DESIGN.md §2.19): x[2 gi] + i x[2 gi + 1], one aligned 16-byte word; values at or beyond n read as 0 (the
// pair whose first value is x[n - 1] keeps it and reads 0 for its second).
template <bool CX>
__device__ __forceinline__ double2 enc_slot(const double* __restrict__ x, uint64_t n, uint64_t gi) {
  if constexpr (CX) {
    if (2 * gi + 1 < n) return reinterpret_cast<const double2*>(x)[gi];
    return make_double2(2 * gi < n ? x[2 * gi] : 0.0, 0.0);
  } else {
    return make_double2(gi < n ? x[gi] : 0.0, 0.0);
  }
}

// (the three kernels that read x are bodies shared by a real and a complex (_cx) entry point, so the real
// forms keep their names and their code)
template <int LOGR, bool CX>
__device__ __forceinline__ void fft_inv_cols_body(const double* __restrict__ x, uint64_t n,
                                                  double2* __restrict__ buf, uint32_t logS,
                                                  const double2* __restrict__ tw) {
  constexpr int R = 1 << LOGR;
  const uint32_t S = 1u << logS;
  const uint32_t BLK = S >> LOGR;
  const uint32_t bpp = BLK / 256;
  const uint64_t k = blockIdx.x / bpp;
  const uint32_t col = (blockIdx.x % bpp) * 256 + threadIdx.x;
  double2 v[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint64_t gi = k * S + col + (uint64_t)r * BLK;
    v[r] = enc_slot<CX>(x, n, gi);
  }
#pragma unroll
  for (int s = 0; s < LOGR; ++s) {
    const uint32_t len = S >> s, lenh = len >> 1;
    const int trr = R >> (s + 1);
#pragma unroll
    for (int r0 = 0; r0 < R; ++r0) {
      if ((r0 / trr) % 2) continue;
      const int r1 = r0 + trr;
      // (col + r0 BLK) mod len, written so rows sharing a twiddle share its load
      const uint32_t j = col + (uint32_t)(r0 & ((R >> s) - 1)) * BLK;
      const double2 W = tw[lenh + j];
      const double2 u = cadd(v[r0], v[r1]);
      const double2 d = csub(v[r0], v[r1]);
      v[r0] = u;
      v[r1] = cmul(d, W);
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) buf[k * S + col + (uint64_t)r * BLK] = v[r];
}
template <int LOGR>
__global__ __launch_bounds__(256) void fft_inv_cols(const double* __restrict__ x, uint64_t n,
                                                    double2* __restrict__ buf, uint32_t logS,
                                                    const double2* __restrict__ tw) {
  fft_inv_cols_body<LOGR, false>(x, n, buf, logS, tw);
}
template <int LOGR>
__global__ __launch_bounds__(256) void fft_inv_cols_cx(const double* __restrict__ x, uint64_t n,
                                                       double2* __restrict__ buf, uint32_t logS,
                                                       const double2* __restrict__ tw) {
  fft_inv_cols_body<LOGR, true>(x, n, buf, logS, tw);
}

template <bool CX>
__device__ __forceinline__ void fft_inv_blocks_body(const double* __restrict__ x, uint64_t n,
                                                    double2* __restrict__ buf, uint32_t logS,
                                                    uint32_t blkLog, int from_x,
                                                    const double2* __restrict__ tw) {
  extern __shared__ __attribute__((aligned(16))) double2 smc[];
  const uint32_t S = 1u << logS, blk = 1u << blkLog;
  const uint32_t sh = logS - blkLog;
  const uint64_t k = blockIdx.x >> sh;
  const uint32_t b = blockIdx.x & ((1u << sh) - 1);
  const uint64_t off = k * S + ((uint64_t)b << blkLog);
  for (uint32_t i = threadIdx.x; i < blk; i += 256) {
    if (from_x) {
      const uint64_t gi = off + i;
      smc[i] = enc_slot<CX>(x, n, gi);
    } else {
      smc[i] = buf[off + i];
    }
  }
  __syncthreads();
  for (uint32_t len = blk; len >= 2; len >>= 1) {
    const uint32_t lenh = len >> 1;
    for (uint32_t p = threadIdx.x; p < blk / 2; p += 256) {
      const uint32_t j = p & (lenh - 1);
      const uint32_t i0 = (p - j) * 2 + j;
      const double2 W = tw[lenh + j];
      const double2 a0 = smc[i0], a1 = smc[i0 + lenh];
      smc[i0] = cadd(a0, a1);
      smc[i0 + lenh] = cmul(csub(a0, a1), W);
    }
    __syncthreads();
  }
  for (uint32_t i = threadIdx.x; i < blk; i += 256) buf[off + i] = smc[i];
}
__global__ __launch_bounds__(256) void fft_inv_blocks(const double* __restrict__ x, uint64_t n,
                                                      double2* __restrict__ buf, uint32_t logS,
                                                      uint32_t blkLog, int from_x,
                                                      const double2* __restrict__ tw) {
  fft_inv_blocks_body<false>(x, n, buf, logS, blkLog, from_x, tw);
}
__global__ __launch_bounds__(256) void fft_inv_blocks_cx(const double* __restrict__ x, uint64_t n,
                                                         double2* __restrict__ buf, uint32_t logS,
                                                         uint32_t blkLog, int from_x,
                                                         const double2* __restrict__ tw) {
  fft_inv_blocks_body<true>(x, n, buf, logS, blkLog, from_x, tw);
}

// FFTSpecialInv's second pass (encode, after fft_inv_cols): DIF half-sizes 2^(BL-1) .. 1.
template <int BL, int K1, int K2, int K3, int K4, bool SWZ = true>
__global__ __launch_bounds__(1 << (BL - 3)) void fft_inv_blocks_ct(double2* __restrict__ buf, uint32_t logS,
                                                                  const double2* __restrict__ tw) {
  static_assert(K1 + K2 + K3 + K4 == BL, "chunk plan");
  __shared__ __attribute__((aligned(16))) double2 sm[1 << BL];
  const uint32_t S = 1u << logS, sh = logS - BL;
  const uint64_t k = blockIdx.x >> sh;
  const uint32_t b = blockIdx.x & ((1u << sh) - 1);
  double2* __restrict__ g = buf + k * S + ((uint64_t)b << BL);
  const auto lds_ld = [&](uint32_t j) { return sm[fft_swz<SWZ>(j)]; };
  const auto lds_st = [&](uint32_t j, double2 v) { sm[fft_swz<SWZ>(j)] = v; };
  fft_chunk<BL, K1, BL - K1, false>(tw, [&](uint32_t j) { return g[j]; }, lds_st);
  __syncthreads();
  fft_chunk<BL, K2, BL - K1 - K2, false>(tw, lds_ld, lds_st);
  __syncthreads();
  fft_chunk<BL, K3, BL - K1 - K2 - K3, false>(tw, lds_ld, lds_st);
  __syncthreads();
  fft_chunk<BL, K4, 0, false>(tw, lds_ld, [&](uint32_t j, double2 v) { g[j] = v; });
}

// FFTSpecialInv (encode) of one 2^14-slot vector per workgroup: x (n doubles, zero-padded) -> buf [K][S].
template <bool CX>
__device__ __forceinline__ void fft_inv_whole_body(const double* __restrict__ x, uint64_t n,
                                                   double2* __restrict__ buf, const double2* __restrict__ tw) {
  constexpr uint32_t S = 1u << kFftWholeLogS, BLK = 1024;
  constexpr int R = 16;
  __shared__ double lds[16 * kFftWholeRow];
  const uint64_t k = blockIdx.x;
  const uint32_t T = threadIdx.x, w = T >> 6, l = T & 63;
  double2 a[R];
  // columns: DIF stages len S .. S/8 on column T (fft_inv_cols<4>)
  // (CX: the vector's 2 S values; enc_slot on the vector's own slice keeps 32-bit offsets)
  constexpr uint32_t VS = CX ? 2 * S : S;
  const double* __restrict__ xk = x + k * VS;
  const uint32_t rem = n > k * VS ? (uint32_t)std::min<uint64_t>(n - k * VS, VS) : 0u;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t i = T + (uint32_t)r * BLK;
    if constexpr (CX)
      a[r] = 2 * i + 1 < rem ? reinterpret_cast<const double2*>(xk)[i] : make_double2(2 * i < rem ? xk[2 * i] : 0.0, 0.0);
    else
      a[r] = make_double2(i < rem ? xk[i] : 0.0, 0.0);
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    asm volatile("" ::: "memory");  // each stage's twiddle loads stay in the stage (fft_fwd_whole)
    const uint32_t lenh = (S >> s) >> 1;
    const int trr = R >> (s + 1);
#pragma unroll
    for (int r0 = 0; r0 < R; ++r0) {
      if ((r0 / trr) % 2) continue;
      const int r1 = r0 + trr;
      const double2 W = tw[lenh + T + (uint32_t)(r0 & ((R >> s) - 1)) * BLK];
      const double2 u = cadd(a[r0], a[r1]);
      const double2 d = csub(a[r0], a[r1]);
      a[r0] = u;
      a[r1] = cmul(d, W);
    }
  }
  fft_whole_transpose<true>(a, lds);
  // block w: DIF half-sizes 512 .. 64 on set l (elements l + 64 m), 32 .. 4 on set l (elements
  // 64 (l >> 2) + (l & 3) + 4 m), 2 .. 1 on sets l + 64 q (elements 4 (l + 64 q) + m)
  double* Ls = lds + w * kFftWholeRow;
  fft_dif_set<4, 6>(a, l, tw);
  fft_wave_xch(a, Ls, [&](int m) { return fft_xb3(l, m); }, [&](int m) { return fft_xb2(l, m); });
  fft_dif_set<4, 2>(a, l & 3, tw);
  fft_wave_xch(a, Ls, [&](int m) { return fft_xa2(l, m); }, [&](int m) { return fft_xa1(l, m); });
  double2* __restrict__ g = buf + k * S + (uint64_t)w * BLK;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    double2 c[4] = {a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]};
    fft_dif_set<2, 0>(c, 0u, tw);
#pragma unroll
    for (int m = 0; m < 4; ++m) g[4 * (l + 64 * q) + m] = c[m];
  }
}
__global__ __launch_bounds__(1024) void fft_inv_whole(const double* __restrict__ x, uint64_t n,
                                                      double2* __restrict__ buf, const double2* __restrict__ tw) {
  fft_inv_whole_body<false>(x, n, buf, tw);
}
__global__ __launch_bounds__(1024) void fft_inv_whole_cx(const double* __restrict__ x, uint64_t n,
                                                         double2* __restrict__ buf, const double2* __restrict__ tw) {
  fft_inv_whole_body<true>(x, n, buf, tw);
}

#define FFT_DISPATCH(LOGRV, KERNEL, ...)                                                   \
  switch (LOGRV) {                                                                       \
    case 1: hipLaunchKernelGGL(KERNEL<1>, __VA_ARGS__); break;                           \
    case 2: hipLaunchKernelGGL(KERNEL<2>, __VA_ARGS__); break;                           \
    case 3: hipLaunchKernelGGL(KERNEL<3>, __VA_ARGS__); break;                           \
    case 4: hipLaunchKernelGGL(KERNEL<4>, __VA_ARGS__); break;                           \
    case 5: hipLaunchKernelGGL(KERNEL<5>, __VA_ARGS__); break;                           \
    case 6: hipLaunchKernelGGL(KERNEL<6>, __VA_ARGS__); break;                           \
    default: throw Error{SHELFI_ERR_ARG, "unsupported batch size"};                      \
  }

// -------------------------------------------------------------- encrypt ----
// One thread = sample group h of a ciphertext: the 16 coefficients j = h + (N/16) i of the
// v2 sampler stream (dev_common.h), so every store is a coalesced row.
// m_j = llround(FFTinv(x)[bitrev(i)] / S * Delta) at j = i*gap (real part) and
// N/2 + i*gap (imaginary part) (CKKSPackedEncoding::Encode layout).  Output is the
// compact per-coefficient record {int64 m + e0, int16 (e1 << 8) | (uint8)v} — 10 bytes
// instead of the 3 L residues the NTT needs, which ntt_fwd_cols_enc expands per tower.
// Encode's range flag (GenFlag words): [0] = a |x Delta| above 2^61 (a finite one: the call is redone on
// the large-value path, launch_encrypt_approx), [1] = a non-finite value (refused).
__device__ __forceinline__ void enc_range_flag(GenFlag f, double val) {
  gen_flag_set(f, 0);
  if (!isfinite(val)) gen_flag_set(f, 1);
}

__global__ __launch_bounds__(256) void enc_prep_kernel(const double2* __restrict__ fbuf,
                                                       uint64_t K, uint32_t logN, uint32_t logS,
                                                       double delta,
                                                       const uint64_t* __restrict__ cdt, int T,
                                                       Key8 key, uint64_t g0,
                                                       int64_t* __restrict__ me0,
                                                       int16_t* __restrict__ ve,
                                                       GenFlag flag) {
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
  const double lim = 2305843009213693952.0;  // 2^61: beyond, the call is redone by launch_encrypt_approx
  uint32_t w[16];
  chacha20_block32(key, h >> 2, nonce, w);
  uint32_t u[4] = {w[4 * (h & 3)], w[4 * (h & 3) + 1], w[4 * (h & 3) + 2], w[4 * (h & 3) + 3]};
  int32_t vv[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) vv[i] = (int32_t)trit_next(u) - 1;
  chacha20_block32(key, V0 + h, nonce, w);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint32_t j = h + N16 * i;
    const uint32_t jj = j < half ? j : j - half;
    int64_t m = 0;
    if ((jj & ((1u << gapLog) - 1)) == 0) {
      const double2 cv = fbuf[k * S + bitrev_dev(jj >> gapLog, logS)];
      const double val = __dmul_rn(__ddiv_rn(j < half ? cv.x : cv.y, dS), delta);
      if (!(fabs(val) <= lim)) enc_range_flag(flag, val);
      m = round_half_away(val);
    }
    me0[(k << logN) + j] = m + gauss32(w[i], thi, tlo, [&] { return chacha20_word(key, V0 + 2 * N16 + h, nonce, i); });
  }
  chacha20_block32(key, V0 + N16 + h, nonce, w);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int32_t e1 =
        (int32_t)gauss32(w[i], thi, tlo, [&] { return chacha20_word(key, V0 + 3 * N16 + h, nonce, i); });
    ve[(k << logN) + h + N16 * i] = (int16_t)((e1 << 8) | (vv[i] & 0xFF));
  }
}

// Encrypt's first NTT pass reading the compact sample record (enc_prep_kernel):
// thread = column c of ciphertext k, coefficients j = c + BLK r.  For every tower the
// three polynomials v, m + e0, e1 are reduced, run through the first LOGR stages and
// stored lazily ([0, 8q)) into pbuf [K][3][L][N] for ntt_fwd_blocks_enc.
template <int LOGR, int POLY>
__global__ __launch_bounds__(256) void ntt_fwd_cols_enc(const int64_t* __restrict__ me0,
                                                        const int16_t* __restrict__ ve, uint64_t K,
                                                        uint32_t logN, uint32_t L,
                                                        const TowerConst* __restrict__ tcs,
                                                        const uint64_t* __restrict__ tw,
                                                        const uint64_t* __restrict__ twp,
                                                        uint64_t* __restrict__ out) {
  constexpr int R = 1 << LOGR;
  const uint32_t BLK = (1u << logN) >> LOGR;
  const uint32_t bpp = BLK / 256;
  const uint64_t k = blockIdx.x / bpp;
  if (k >= K) return;
  const uint32_t c = (blockIdx.x % bpp) * 256 + threadIdx.x;
  const uint64_t LN = (uint64_t)L << logN;
  const uint64_t j0 = (k << logN) + c;
  // POLY: 0 = v, 1 = m + e0, 2 = e1 (one launch each).  The record is re-read for every
  // tower (L1/L2 hits) rather than kept live beside the R residues: keeping R int64
  // sources across the tower loop cost 2 waves/SIMD of occupancy (170 VGPRs).
#pragma unroll 1
  for (uint32_t t = 0; t < L; ++t) {
    const TowerConst cst = tcs[t];
    const uint64_t q = cst.q;
    const uint64_t* __restrict__ w = tw + ((uint64_t)t << logN);
    const uint64_t* __restrict__ wp = twp + ((uint64_t)t << logN);
    uint64_t x[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const uint64_t j = j0 + (uint64_t)BLK * r;
      if (POLY == 1) {
        x[r] = mod_signed_dev(me0[j], cst);
        if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // bound reductions in flight
      } else {
        const int32_t sv = ve[j];
        x[r] = small_mod(POLY == 0 ? (int32_t)(int8_t)(sv & 0xFF) : (sv >> 8), q);
      }
    }
#pragma unroll
    for (int s = 0; s < LOGR; ++s) {
      const int m = 1 << s, tr = R >> (s + 1);
#pragma unroll
      for (int i = 0; i < m; ++i) {
        const uint64_t W = w[m + i], Wp = wp[m + i];
#pragma unroll
        for (int jj = 0; jj < tr; ++jj) {
          const int r0 = 2 * i * tr + jj, r1 = r0 + tr;
          if (fwd_red_at(s))
            ct_bfly_s<true>(x[r0], x[r1], W, Wp, q, cst.n8q);
          else
            ct_bfly_s<false>(x[r0], x[r1], W, Wp, q, cst.n8q);
        }
      }
    }
    uint64_t* __restrict__ o = out + (k * 3 + POLY) * LN + ((uint64_t)t << logN) + c;
    // the blocks passes take inputs below 8q
#pragma unroll
    for (int r = 0; r < R; ++r) o[(uint64_t)r * BLK] = fwd_bound(LOGR) > 8 ? csub_neg(x[r], cst.n8q) : x[r];
  }
}

// Encode + sampling + the columns pass in one kernel (enc_prep_kernel followed by the three
// ntt_fwd_cols_enc launches, without the 10-byte-per-coefficient record in between):
// thread = column c of ciphertext k, coefficients j = c + BLK r (r < R = 2^LOGR).  In the v2
// sampler stream (dev_common.h) coefficient j = h + (N/16) i: the column's rows are the sample
// indices i = i0 + (16/R) r of group h = c mod N/16 (i0 = c div N/16; LOGR = 4: the whole group).
// Same samples and rounding as enc_prep_kernel, then for every tower the columns stages of v,
// m + e0 and e1 and the lazy stores into pbuf that the blocks pass reads.
// WV: waves per SIMD the register budget is cut for.  TWL: the tower's column-stage twiddles are
// staged in LDS per tower instead of scalar-loaded (the scalar loads of 15 {w, w'} pairs per polynomial
// were spilling SGPRs).
// TS (round 4, small batches): wave w of a workgroup takes tower w (L = 4) of 64 columns, each wave
// sampling its columns itself (4x the sampler work, no cross-wave traffic): a K = 4 call's 8192
// columns become 512 waves instead of 128, for calls too small to fill the chip one column per thread
// (register budget for 2 waves per SIMD: a small call has no more to give it).
// VT (round 5; LOGR = 4, TAB, not TS): v's columns pass is left to the blocks pass, which sums
// DeviceTables::enc_vtab entries for each row; this kernel writes only the column's 4 radix-4 group
// patterns, packed 7 bits each into one uint32 at word c of the ciphertext's pbuf v region (8 KiB per
// ciphertext instead of v's 4 towers x 256 KiB).
// X5 (round 6; LOGR = 4, not TS / VT): one more columns stage for rings whose blocks pass starts at
// global stage 5 (2^16 over 2^11 blocks, nlogR = 5).  A workgroup's threads hold columns c (tid < 128)
// and c + BLK/2 (tid >= 128) of the 16-row decomposition; stage 4 pairs row r of the two (twiddle
// psi_rev[16 + r]), so after the register stages each thread trades 8 rows with its partner through
// LDS and runs 8 of the 16 butterflies: the low thread keeps rows 0-7 of both columns, the high one
// rows 8-15.  pbuf then holds what a 32-row columns pass leaves, without 32-row register columns.
template <int LOGR, bool TAB, int WV = 4, bool TWL = false, bool TS = false, bool VT = false, bool X5 = false>
__global__ __launch_bounds__(256, TS ? 2 : WV) void enc_cols_fused(const double2* __restrict__ fbuf, uint64_t K,
                                                      uint32_t logN, uint32_t logS, uint32_t L,
                                                      double delta, const uint64_t* __restrict__ cdt,
                                                      int T, Key8 key, uint64_t g0,
                                                      const TowerConst* __restrict__ tcs,
                                                      const uint64_t* __restrict__ tw,
                                                      const uint64_t* __restrict__ twp,
                                                      uint64_t* __restrict__ out,
                                                      GenFlag flag, uint32_t t_split,
                                                      const uint64_t* __restrict__ enc_tab) {
  constexpr int R = 1 << LOGR, IS = 16 / R, G = R / 4;
  constexpr int NTW = TS ? 4 : 1;  // towers with their own LDS tables in one workgroup
  static_assert(LOGR == 3 || LOGR == 4, "a column is 8 or 16 rows of one sample group");
  static_assert(!VT || (LOGR == 4 && TAB && !TS), "v tables: 16-row columns, one column per thread");
  static_assert(!X5 || (LOGR == 4 && TAB && !TS && !VT), "the exchanged stage: 16-row columns, one per thread");
  constexpr int NTWL = X5 ? 2 << LOGR : 1 << LOGR;  // column-stage twiddles psi_rev[1 .. NTWL)
  __shared__ uint32_t thi[64], tlo[64];
  __shared__ uint64_t tabs_all[NTW][kEncTab];  // the tower's DeviceTables::enc_tab slice
  __shared__ ulonglong2 twl_all[NTW][NTWL];  // TWL: the tower's {w, w'} for column stages (index m + i)
  __shared__ uint64_t xch[X5 ? 8 * 256 : 1];   // X5: the 8 rows a thread trades, [row][thread]
  static_assert(!TWL || TAB, "LDS twiddles ride on the table path's per-tower barrier");
  const uint32_t wave = TS ? (threadIdx.x >> 6) : 0u, tid = TS ? (threadIdx.x & 63u) : threadIdx.x;
  uint64_t* tabs = tabs_all[wave];
  ulonglong2* twl = twl_all[wave];
  // TS: each wave's tables are its own, so ordering its LDS writes before its reads needs no barrier
  const auto tower_sync = [] {
    if (TS)
      wave_lds_sync();
    else
      __syncthreads();
  };
  load_cdt32(cdt, T, thi, tlo);
  __syncthreads();
  const uint32_t N = 1u << logN, BLK = N >> LOGR, N16 = N >> 4, V0 = N >> 6;
  const uint64_t gid = TS ? (uint64_t)blockIdx.x * 64 + tid : (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t k = gid >> (logN - LOGR);
  if (k >= K) return;  // workgroup-uniform (BLK is a multiple of 256)
  // X5: workgroup wi of a ciphertext holds column pairs (wi 128 + l, wi 128 + l + BLK/2), l < 128
  const uint32_t c = X5 ? (((uint32_t)(gid & (BLK - 1)) >> 8) << 7) + (threadIdx.x & 127u) +
                              ((threadIdx.x >> 7) ? (BLK >> 1) : 0u)
                        : (uint32_t)(gid & (BLK - 1));
  const uint32_t h = c & (N16 - 1), i0 = c >> (logN - 4);
  const uint64_t nonce = (1ull << 56) | (g0 + k);
  const uint32_t S = 1u << logS, gapLog = logN - 1 - logS;
  const double invS = 1.0 / (double)S;  // a power of two: x * (1/S) == x / S exactly
  const double lim = 2305843009213693952.0;  // 2^61: beyond, the call is redone by launch_encrypt_approx
  const uint64_t LN = (uint64_t)L << logN;
  // columns stages of one polynomial of tower t (values x[r] < q) and its lazy store
  // (towers with q < kNoRedQ run unreduced (NORED, fwd_set_ct): no stage reductions, no
  // store reduction; the blocks pass knows)
  // (first: the stage the values enter at; the small polynomials skip stages their tables did)
  auto cols = [&](uint64_t (&x)[R], uint32_t t, const TowerConst& cst, int poly, auto nored, auto first)
                  __attribute__((always_inline)) {
    constexpr bool NR = decltype(nored)::value;
    const uint64_t q = cst.q;
    const uint64_t* __restrict__ w = tw + ((uint64_t)t << logN);
    const uint64_t* __restrict__ wp = twp + ((uint64_t)t << logN);
#pragma unroll
    for (int s = decltype(first)::value; s < LOGR; ++s) {
      const int m = 1 << s, tr = R >> (s + 1);
#pragma unroll
      for (int i = 0; i < m; ++i) {
        uint64_t W, Wp;
        if constexpr (TWL) {
          const ulonglong2 T2 = twl[m + i];
          W = T2.x;
          Wp = T2.y;
        } else {
          W = w[m + i];
          Wp = wp[m + i];
        }
#pragma unroll
        for (int jj = 0; jj < tr; ++jj) {
          const int r0 = 2 * i * tr + jj, r1 = r0 + tr;
          if (!NR && fwd_red_at(s))
            ct_bfly_s<true>(x[r0], x[r1], W, Wp, q, cst.n8q);
          else
            ct_bfly_s<false>(x[r0], x[r1], W, Wp, q, cst.n8q);
        }
      }
    }
    uint64_t* __restrict__ o = out + (k * 3 + poly) * LN + ((uint64_t)t << logN) + c;
    if constexpr (X5) {
      // stage LOGR: row r of column c (low thread) with row r of c + BLK/2 (high thread), twiddle
      // psi_rev[R + r]; each keeps 8 rows of both columns
      const bool lo = threadIdx.x < 128;  // wave-uniform
      __syncthreads();                    // the previous exchange's reads are done
      // (explicit wave-uniform branches: a select between two register elements becomes a select
      // of addresses, which puts the array in scratch)
      if (lo) {
#pragma unroll
        for (int r = 0; r < R / 2; ++r) xch[r * 256 + threadIdx.x] = x[R / 2 + r];
      } else {
#pragma unroll
        for (int r = 0; r < R / 2; ++r) xch[r * 256 + threadIdx.x] = x[r];
      }
      __syncthreads();
      uint64_t y[R / 2];
#pragma unroll
      for (int r = 0; r < R / 2; ++r) y[r] = xch[r * 256 + (threadIdx.x ^ 128u)];
      constexpr bool RD = fwd_red_at(LOGR);
      const uint32_t rb = lo ? 0u : (uint32_t)(R / 2);  // this thread's rows rb .. rb + 7
      const int64_t dpart = lo ? (int64_t)(BLK >> 1) : -(int64_t)(BLK >> 1);  // the partner column
#pragma unroll
      for (int r = 0; r < R / 2; ++r) {
        uint64_t W, Wp;
        if constexpr (TWL) {
          const ulonglong2 T2 = twl[R + rb + r];
          W = T2.x;
          Wp = T2.y;
        } else {
          W = w[R + rb + r];
          Wp = wp[R + rb + r];
        }
        // low: (x[r], y[r]) = (c, c + BLK/2) at row r; high: (y[r], x[8 + r]) = (c - BLK/2, c) at row 8 + r
        // (wave-uniform branches with static register indices)
        if (lo)
          ct_bfly_s<!NR && RD>(x[r], y[r], W, Wp, q, cst.n8q);
        else
          ct_bfly_s<!NR && RD>(y[r], x[R / 2 + r], W, Wp, q, cst.n8q);
      }
      const auto fin = [&](uint64_t v) { return (!NR && fwd_bound(LOGR + 1) > 8) ? csub_neg(v, cst.n8q) : v; };
      if (lo) {
#pragma unroll
        for (int r = 0; r < R / 2; ++r) {
          o[(uint64_t)r * BLK] = fin(x[r]);          // own column
          o[(uint64_t)r * BLK + dpart] = fin(y[r]);  // the partner's column
        }
      } else {
#pragma unroll
        for (int r = 0; r < R / 2; ++r) {
          o[(uint64_t)(R / 2 + r) * BLK] = fin(x[R / 2 + r]);
          o[(uint64_t)(R / 2 + r) * BLK + dpart] = fin(y[r]);
        }
      }
      return;
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
      o[(uint64_t)r * BLK] = (!NR && fwd_bound(LOGR) > 8) ? csub_neg(x[r], cst.n8q) : x[r];
  };
  // phase 1: v (16 digits of a 128-bit word group) and e1, packed (e1 << 8) | (uint8) v
  {
    int32_t sv[R];
    {
      // block h/4 is shared by the quad of lanes h & ~3 .. h | 3 (h mod 4 = lane mod 4)
      uint32_t u[4];
      chacha20_quad(key, h >> 2, nonce, u);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int32_t d = (int32_t)trit_next(u) - 1;
        if (IS == 1) {
          sv[i] = d & 0xFF;
        } else if ((i % IS) == 0) {
          if (i0 == 0) sv[i / IS] = d & 0xFF;
        } else if (i0 == 1) {
          sv[i / IS] = d & 0xFF;
        }
      }
    }
    {
      uint32_t we[16];
      chacha20_block32(key, V0 + N16 + h, nonce, we);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const uint32_t i = IS == 1 ? (uint32_t)r : i0 + IS * r;
        const uint32_t wi = IS == 1 ? we[r] : (i0 ? we[IS * r + 1] : we[IS * r]);  // no dynamic register index
        sv[r] |= (int32_t)gauss32(wi, thi, tlo, [&] { return chacha20_word(key, V0 + 3 * N16 + h, nonce, i); }) << 8;
      }
    }
    // v's first two column stages are table lookups: rows g, g + R/4, g + R/2, g + 3R/4 (g < R/4)
    // form a radix-4 group whose 4 outputs depend only on its 4 ternary inputs (81 patterns,
    // DeviceTables::enc_tab, canonical); e1's stage 0 reads W0 e from the table (|e| <= 63).
    // The canonical ciphertext is the same; only lazy intermediates differ (smaller bounds).
    uint32_t vidx[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const auto tr = [&](int r) { return (uint32_t)((int32_t)(int8_t)(sv[r] & 0xFF) + 1); };
      vidx[g] = tr(g) + 3 * tr(g + G) + 9 * tr(g + 2 * G) + 27 * tr(g + 3 * G);
    }
    if constexpr (VT)
      reinterpret_cast<uint32_t*>(out + k * 3 * LN)[c] = vidx[0] | (vidx[1] << 7) | (vidx[2] << 14) | (vidx[3] << 21);
    // towers [0, t_split) reduced, [t_split, L) unreduced (q < kNoRedQ; the blocks pass knows)
    const auto small_polys = [&](uint32_t ta, uint32_t tb, auto nored) __attribute__((always_inline)) {
#pragma unroll 1
      for (uint32_t t = ta; t < tb; ++t) {
        if (TS && t != wave) continue;  // wave-uniform
        const TowerConst cst = tcs[t];
        if constexpr (!TAB) {  // A/B reference: every stage as butterflies (SHELFI_ENC_TAB=0)
#pragma unroll 1
          for (int poly = 0; poly < 3; poly += 2) {
            uint64_t x[R];
#pragma unroll
            for (int r = 0; r < R; ++r)
              x[r] = small_mod(poly == 0 ? (int32_t)(int8_t)(sv[r] & 0xFF) : (sv[r] >> 8), cst.q);
            cols(x, t, cst, poly, nored, std::integral_constant<int, 0>{});
          }
          continue;
        }
        tower_sync();  // the previous tower's lookups are done (every thread runs every tower)
        for (uint32_t i = tid; i < (uint32_t)kEncTab; i += (TS ? 64u : 256u)) tabs[i] = enc_tab[(size_t)t * kEncTab + i];
        if constexpr (TWL) {
          if (tid < (uint32_t)NTWL)
            twl[tid] = make_ulonglong2(tw[((uint64_t)t << logN) + tid], twp[((uint64_t)t << logN) + tid]);
        }
        tower_sync();
        if constexpr (!VT) {
          uint64_t x[R];
#pragma unroll
          for (int g = 0; g < G; ++g)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) x[g + kk * G] = tabs[kk * 81 + vidx[g]];
          cols(x, t, cst, 0, nored, std::integral_constant<int, 2>{});
        }
        {
          uint64_t x[R];
#pragma unroll
          for (int r = 0; r < R / 2; ++r) {
            const uint64_t xa = small_mod(sv[r] >> 8, cst.q);
            const uint64_t tt = tabs[kEncVTab + 64 + (sv[r + R / 2] >> 8)];  // W0 e mod q
            x[r] = xa + tt;                   // < 2q
            x[r + R / 2] = xa + cst.q - tt;   // (0, 2q)
          }
          cols(x, t, cst, 2, nored, std::integral_constant<int, 1>{});
        }
      }
    };
    small_polys(0, t_split, std::false_type{});
    small_polys(t_split, L, std::true_type{});
  }
  // phase 2: m + e0; rows r and r + R/2 are the real and imaginary parts of one slot
  int64_t me[R];
  {
    uint32_t we[16];
    chacha20_block32(key, V0 + h, nonce, we);
#pragma unroll
    for (int r = 0; r < R / 2; ++r) {
      const uint32_t jj = c + BLK * r;  // < N/2
      int64_t mre = 0, mim = 0;
      if ((jj & ((1u << gapLog) - 1)) == 0) {
        const double2 cv = fbuf[k * S + bitrev_dev(jj >> gapLog, logS)];
        const double vr = __dmul_rn(__dmul_rn(cv.x, invS), delta);
        const double vi = __dmul_rn(__dmul_rn(cv.y, invS), delta);
        if (!(fabs(vr) <= lim) || !(fabs(vi) <= lim)) {
          gen_flag_set(flag, 0);
          if (!isfinite(vr) || !isfinite(vi)) gen_flag_set(flag, 1);
        }
        mre = round_half_away(vr);
        mim = round_half_away(vi);
      }
#pragma unroll
      for (int part = 0; part < 2; ++part) {
        const int rr = r + part * (R / 2);
        const uint32_t i = IS == 1 ? (uint32_t)rr : i0 + IS * rr;
        const uint32_t wi = IS == 1 ? we[rr] : (i0 ? we[IS * rr + 1] : we[IS * rr]);
        me[rr] = (part ? mim : mre) +
                 gauss32(wi, thi, tlo, [&] { return chacha20_word(key, V0 + 2 * N16 + h, nonce, i); });
      }
    }
  }
  // The first columns stage pairs rows r and r + R/2 and reads the upper row only through its
  // lazy Shoup product, which takes any 64-bit multiplicand: rows >= R/2 enter as
  // u = m + e0 + floor(2^62 / q) q (in [0, 2^63), congruent), and only rows < R/2 are reduced
  // (red_any, q >= 2^40).  The canonical ciphertext is the same; only lazy intermediates differ.
  const auto message_poly = [&](uint32_t ta, uint32_t tb, auto nored) __attribute__((always_inline)) {
#pragma unroll 1
    for (uint32_t t = ta; t < tb; ++t) {
      if (TS && t != wave) continue;  // wave-uniform
      if constexpr (TWL) {
        tower_sync();  // every thread runs every tower
        if (tid < (uint32_t)NTWL)
          twl[tid] = make_ulonglong2(tw[((uint64_t)t << logN) + tid], twp[((uint64_t)t << logN) + tid]);
        tower_sync();
      }
      const TowerConst cst = tcs[t];
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
      cols(x, t, cst, 1, nored, std::integral_constant<int, 0>{});
    }
  };
  message_poly(0, t_split, std::false_type{});
  message_poly(t_split, L, std::true_type{});
}

// Encrypt's last NTT pass fused with the public-key combine: one workgroup owns block
// b of tower t of ciphertext k, transforms v, m + e0 and e1 (pbuf [K][3][L][N], lazy
// after the columns pass) one after the other through the same LDS block, and writes
// c0 = v*b + (m + e0), c1 = v*a + e1 (ckks.cpp:81, PALISADE Encrypt) — the transformed
// polynomials never return to HBM.
template <int PP>  // 16-byte pairs per thread: blk / 512
__global__ __launch_bounds__(256) void ntt_fwd_blocks_enc(const uint64_t* __restrict__ pbuf,
                                                          uint32_t L, uint32_t logN, uint32_t sstart,
                                                          const uint64_t* __restrict__ tw,
                                                          const uint64_t* __restrict__ twp,
                                                          const TowerConst* __restrict__ tcs,
                                                          const uint64_t* __restrict__ pk,
                                                          const uint64_t* __restrict__ pksh,
                                                          uint64_t* __restrict__ ct,
                                                          const int64_t* __restrict__ me0,
                                                          const int16_t* __restrict__ ve) {
  extern __shared__ __attribute__((aligned(16))) uint64_t sm[];
  const uint32_t blkLog = logN - sstart, blk = 1u << blkLog;
  const uint32_t b = blockIdx.x & ((1u << sstart) - 1);
  const uint64_t rest = blockIdx.x >> sstart;
  const uint32_t t = (uint32_t)(rest % L);
  const uint64_t k = rest / L;
  const uint64_t q = tcs[t].q;
  const uint64_t* __restrict__ w = tw + ((uint64_t)t << logN);
  const uint64_t* __restrict__ wp = twp + ((uint64_t)t << logN);
  const uint64_t off = ((uint64_t)t << logN) + ((uint64_t)b << blkLog);  // within [L][N]
  const uint64_t LN = (uint64_t)L << logN;
  ulonglong2 V[PP];  // NTT(v), kept for both products
#pragma unroll
  for (int poly = 0; poly < 3; ++poly) {
    if (me0) {  // single-pass ring: expand the compact sample record (no columns pass)
      const TowerConst& cst = tcs[t];
      const uint64_t base = (k << logN) + ((uint64_t)b << blkLog);
      for (uint32_t i = threadIdx.x; i < blk; i += 256) {
        const int32_t sv = ve[base + i];
        sm[lds_sw(i)] = poly == 1 ? mod_signed_dev(me0[base + i], cst)
                                  : small_mod(poly == 0 ? (int32_t)(int8_t)(sv & 0xFF) : (sv >> 8), q);
      }
    } else {
      const ulonglong2* src = reinterpret_cast<const ulonglong2*>(pbuf + (k * 3 + poly) * LN + off);
      for (uint32_t p = threadIdx.x; p < blk / 2; p += 256) lds_put2(sm, p, src[p]);
    }
    __syncthreads();
    ntt_fwd_block_stages(sm, blkLog, b, logN, w, wp, q);
#pragma unroll
    for (int i = 0; i < PP; ++i) {
      const uint32_t p = threadIdx.x + 256 * i;
      if (p >= blk / 2) break;
      ulonglong2 v = lds_get2(sm, p);
      v = make_ulonglong2(canon8(v.x, q), canon8(v.y, q));
      const uint64_t e = off + 2 * p;
      if (poly == 0) {
        V[i] = v;
      } else {  // poly 1: c0 = v*b + (m + e0); poly 2: c1 = v*a + e1
        const uint64_t off_pk = (poly == 1 ? 0 : LN) + e;
        const ulonglong2 P = *reinterpret_cast<const ulonglong2*>(pk + off_pk);
        const ulonglong2 Ps = *reinterpret_cast<const ulonglong2*>(pksh + off_pk);
        ulonglong2 c;
        c.x = addmod(shoup_mul(V[i].x, P.x, Ps.x, q), v.x, q);
        c.y = addmod(shoup_mul(V[i].y, P.y, Ps.y, q), v.y, q);
        *reinterpret_cast<ulonglong2*>(ct + (k * 2 + (poly - 1)) * LN + e) = c;
      }
    }
    __syncthreads();  // LDS is refilled by the next polynomial
  }
}

// Encrypt's blocks pass at compile-time shape: chunks K1..K4 (sum BL) per polynomial,
// the first on registers loaded straight from pbuf, the last combined with the public key straight
// from registers (3 LDS round trips and 3 barriers per polynomial instead of 5 and 5).
// Same contract as ntt_fwd_blocks_enc.
template <int BL, int K1, int K2, int K3, int K4>
__global__ __launch_bounds__(256) void ntt_fwd_blocks_enc_ct(
    const uint64_t* __restrict__ pbuf, uint32_t L, uint32_t logN, const ulonglong2* __restrict__ twb,
    const TowerConst* __restrict__ tcs, const uint64_t* __restrict__ pk,
    const uint64_t* __restrict__ pksh, uint64_t* __restrict__ ct, uint32_t zero, uint32_t xg) {
  static_assert(K1 + K2 + K3 + K4 == BL, "chunk plan must cover the block");
  constexpr int M1 = 1 << K1, NS1 = (1 << (BL - K1)) / 256, D1 = BL - K1;
  constexpr int ML = 1 << K4, NSL = (1 << (BL - K4)) / 256;
  __shared__ __attribute__((aligned(16))) uint64_t sm[lpad_size(BL)];
  const uint32_t sstart = logN - BL;
  const uint32_t bid = xcd_block(blockIdx.x, xg);
  const uint32_t b = bid & ((1u << sstart) - 1);
  const uint32_t rest = bid >> sstart;
  const uint32_t t = rest % L, k = rest / L;
  const TowerConst& cst = tcs[t];
  const uint64_t q = cst.q, n8q = cst.n8q;
  const ulonglong2* tb0 = twb + ((uint64_t)t << logN) + ((uint64_t)b << BL);
  const uint64_t off = ((uint64_t)t << logN) + ((uint64_t)b << BL);
  const uint64_t LN = (uint64_t)L << logN;
  const auto lds_ld = [&](uint32_t, uint32_t pj) { return sm[pj]; };
  uint64_t V[NSL][ML];  // NTT(v) at this thread's last-chunk positions
#pragma unroll 1
  for (int poly = 0; poly < 3; ++poly) {
    // reload the twiddles per polynomial (zero == 0 is opaque to the compiler): hoisted
    // out of this loop they would hold ~100 VGPRs for the whole kernel
    const ulonglong2* __restrict__ tb = tb0 + poly * zero;
    const uint64_t* __restrict__ src = pbuf + ((uint64_t)k * 3 + poly) * LN + off;
#pragma unroll
    for (int r = 0; r < NS1; ++r) {  // first chunk: one group, block-uniform twiddles
      uint64_t x[M1];
#pragma unroll
      for (int m = 0; m < M1; ++m) x[m] = src[threadIdx.x + 256u * r + (m << D1)];
      fwd_set_ct<BL, BL - 1, K1>(x, 0u, tb, q, n8q);
      const uint32_t p0 = lpad(threadIdx.x + 256u * r);
#pragma unroll
      for (int m = 0; m < M1; ++m) sm[p0 + lofs<(1 << D1)>(m)] = x[m];
    }
    __syncthreads();
    fwd_chunk_ct<BL, BL - 1 - K1, K2>(tb, q, n8q, lds_ld, [&](int, uint32_t, uint32_t pj0, auto& x) {
#pragma unroll
      for (int m = 0; m < (1 << K2); ++m) sm[pj0 + lofs<(1 << (BL - K1 - K2))>(m)] = x[m];
    });
    __syncthreads();
    fwd_chunk_ct<BL, BL - 1 - K1 - K2, K3>(tb, q, n8q, lds_ld, [&](int, uint32_t, uint32_t pj0, auto& x) {
#pragma unroll
      for (int m = 0; m < (1 << K3); ++m) sm[pj0 + lofs<(1 << (BL - K1 - K2 - K3))>(m)] = x[m];
    });
    __syncthreads();
    // last chunk (contiguous sets of ML, written inline: V captured by a lambda would
    // live in scratch)
#pragma unroll
    for (int r = 0; r < NSL; ++r) {
      const uint32_t g = threadIdx.x + 256u * r, j0 = g << K4, pj0 = lpad(j0);
      uint64_t x[ML];
#pragma unroll
      for (int m = 0; m < ML; ++m) x[m] = sm[pj0 + m];
      fwd_set_ct<BL, K4 - 1, K4>(x, g, tb, q, n8q);
      if (poly == 0) {  // NTT(v), lazy (< 12q): only ever a Shoup multiplicand
#pragma unroll
        for (int m = 0; m < ML; ++m) V[r][m] = x[m];
      } else {  // poly 1: c0 = v*b + (m + e0); poly 2: c1 = v*a + e1 (< 4q + 12q, then [0, q))
        const uint64_t e = off + j0;
        const uint64_t off_pk = (poly == 1 ? 0 : LN) + e;
        uint64_t* __restrict__ dst = ct + ((uint64_t)k * 2 + (poly - 1)) * LN + e;
#pragma unroll
        for (int m = 0; m < ML; m += 2) {
          const ulonglong2 P = *reinterpret_cast<const ulonglong2*>(pk + off_pk + m);
          const ulonglong2 Ps = *reinterpret_cast<const ulonglong2*>(pksh + off_pk + m);
          ulonglong2 c;
          c.x = red_any(shoup_lazy(V[r][m], P.x, Ps.x, q) + x[m], cst);
          c.y = red_any(shoup_lazy(V[r][m + 1], P.y, Ps.y, q) + x[m + 1], cst);
          *reinterpret_cast<ulonglong2*>(dst + m) = c;
        }
      }
    }
    __syncthreads();  // LDS is refilled by the next polynomial
  }
}

// Persistent, software-pipelined form of ntt_fwd_blocks_enc_ct (round 3), the same idea as
// ntt_inv_blocks_dec_pp: a workgroup owns one (tower, block) combo and walks ciphertexts
// k0, k0 + P, ...; the combo's twiddle slice sits in LDS (copied once); each polynomial's
// first-chunk pbuf words are loaded into registers while the previous polynomial is being
// transformed, and the public-key words of the combine are requested one polynomial ahead.
// Same arithmetic and outputs as ntt_fwd_blocks_enc_ct.
// NR: the launch covers towers [t0, t0 + nt) whose columns pass ran unreduced (q < kNoRedQ,
// enc_cols_fused's t_split): no reductions in the block stages either (fwd_set_ct).
// WL (round 4): only the first chunk's exchange crosses waves.  After the stages of half-size
// 2^(BL-1) .. 2^(BL-K1) the block falls apart into 2^K1 independent sub-blocks; the middle chunks'
// sets already keep each wave inside 512 contiguous elements, and the last chunk's sets are dealt
// so that they do too (set g = 2 * 64 w + 64 r + lane), so the exchanges between the middle chunks
// and into the last one need only the wave's own LDS ordering (wave_lds_sync), not a workgroup
// barrier: 2 barriers per polynomial instead of 4.
// VT (round 5): v's columns pass never ran (enc_cols_fused<..., VT>): the first chunk's v words are
// the column's packed group patterns, and each row value is the sum of its block's 4 enc_vtab entries
// (< 4q), looked up in a 2.6 KiB LDS slice copied once per workgroup (the combo's block b is the row).
template <int BL, int K1, int K2, int K3, int K4, bool NR, bool WL = false, bool VT = false>
__global__ __launch_bounds__(256) void ntt_fwd_blocks_enc_pp(
    const uint64_t* __restrict__ pbuf, uint32_t L, uint32_t logN, const ulonglong2* __restrict__ twb,
    const TowerConst* __restrict__ tcs, const uint64_t* __restrict__ pk, const uint64_t* __restrict__ pksh,
    uint64_t* __restrict__ ct, uint32_t K, uint32_t per_combo, uint32_t t0, uint32_t nt,
    const uint64_t* __restrict__ vtab) {
  static_assert(K1 + K2 + K3 + K4 == BL, "chunk plan must cover the block");
  static_assert(!VT || (BL == 11 && K1 == 3), "v tables: a 16-row columns pass, 8 columns per thread");
  constexpr int M1 = 1 << K1, NS1 = (1 << (BL - K1)) / 256, D1 = BL - K1;
  constexpr int ML = 1 << K4, NSL = (1 << (BL - K4)) / 256;
  // WL needs every middle-chunk set of a wave inside its 64 * 2^(BL-8) contiguous elements
  static_assert(!WL || (BL == 11 && K1 == 3 && K2 == 3 && K3 == 3 && K4 == 2), "wave-local plan");
  __shared__ __attribute__((aligned(16))) ulonglong2 tws[1 << BL];
  __shared__ __attribute__((aligned(16))) uint64_t sm[lpad_size(BL)];
  __shared__ uint64_t vts[VT ? 4 * 81 : 1];
  // the last chunk's set r of this thread
  const auto last_g = [&](int r) -> uint32_t {
    return WL ? ((threadIdx.x >> 6) * (64u * NSL) + 64u * r + (threadIdx.x & 63u)) : threadIdx.x + 256u * r;
  };
  const uint32_t sstart = logN - BL;
  const uint32_t ncombo = nt << sstart;
  const uint32_t combo = blockIdx.x % ncombo;
  const uint32_t b = combo & ((1u << sstart) - 1), t = t0 + (combo >> sstart);
  const TowerConst& cst = tcs[t];
  const uint64_t q = cst.q, n8q = cst.n8q;
  const uint64_t off = ((uint64_t)t << logN) + ((uint64_t)b << BL);
  const uint64_t LN = (uint64_t)L << logN;
  {
    const ulonglong2* __restrict__ src = twb + off;
    for (uint32_t i = threadIdx.x; i < (1u << BL); i += 256) tws[i] = src[i];
    if (VT)  // rows = blocks: this combo's row b of tower t
      for (uint32_t i = threadIdx.x; i < 4 * 81; i += 256) vts[i] = vtab[((uint64_t)t * 16 + b) * (4 * 81) + i];
  }
  uint64_t pf[NS1][M1];              // the next polynomial's first-chunk words
  ulonglong2 P[NSL][ML / 2], Ps[NSL][ML / 2];  // the next combine's key words (b or a)
  uint64_t V[NSL][ML];                // NTT(v) at this thread's last-chunk positions
  const auto fetch = [&](uint32_t kk, int poly) {
    if (VT && poly == 0) {  // the packed patterns of columns tid + 256 m (this block's row of each)
      const uint32_t* __restrict__ vp = reinterpret_cast<const uint32_t*>(pbuf + (uint64_t)kk * 3 * LN);
#pragma unroll
      for (int m = 0; m < M1; ++m) pf[0][m] = vp[threadIdx.x + (m << D1)];
      return;
    }
    const uint64_t* __restrict__ src = pbuf + ((uint64_t)kk * 3 + poly) * LN + off;
#pragma unroll
    for (int r = 0; r < NS1; ++r)
#pragma unroll
      for (int m = 0; m < M1; ++m) pf[r][m] = __builtin_nontemporal_load(src + threadIdx.x + 256u * r + (m << D1));
  };
  const auto fetch_key = [&](int poly) {  // poly 1: b, poly 2: a
#pragma unroll
    for (int r = 0; r < NSL; ++r) {
      const uint64_t e = (poly == 1 ? 0 : LN) + off + (last_g(r) << K4);
#pragma unroll
      for (int m = 0; m < ML; m += 2) {
        P[r][m / 2] = *reinterpret_cast<const ulonglong2*>(pk + e + m);
        Ps[r][m / 2] = *reinterpret_cast<const ulonglong2*>(pksh + e + m);
      }
    }
  };
  uint32_t k = blockIdx.x / ncombo;
  if (k < K) fetch(k, 0);
  __syncthreads();  // the twiddle slice is in LDS
  const auto lds_ld = [&](uint32_t, uint32_t pj) { return sm[pj]; };
  const auto mid_sync = [] {
    if (WL)
      wave_lds_sync();
    else
      __syncthreads();
  };
#pragma unroll 1
  for (; k < K; k += per_combo) {
#pragma unroll 1
    for (int poly = 0; poly < 3; ++poly) {
      uint64_t x[NS1][M1];
      if (VT && poly == 0) {  // NTT(v)'s columns pass as table sums: row b of each column, < 4q
#pragma unroll
        for (int m = 0; m < M1; ++m) {
          const uint32_t w = (uint32_t)pf[0][m];
          x[0][m] = vts[w & 127u] + vts[81 + ((w >> 7) & 127u)] + vts[162 + ((w >> 14) & 127u)] + vts[243 + (w >> 21)];
        }
      } else {
#pragma unroll
        for (int r = 0; r < NS1; ++r)
#pragma unroll
          for (int m = 0; m < M1; ++m) x[r][m] = pf[r][m];
      }
      // the next polynomial's words (or the next ciphertext's v) and this one's key words
      if (poly < 2)
        fetch(k, poly + 1);
      else if (k + per_combo < K)
        fetch(k + per_combo, 0);
      if (poly > 0) fetch_key(poly);
#pragma unroll
      for (int r = 0; r < NS1; ++r)  // first chunk: one group, block-uniform twiddles
        fwd_set_ct<BL, BL - 1, K1, NR>(x[r], 0u, tws, q, n8q);
      // WL: the previous polynomial's last-chunk reads must be done before LDS is refilled; with the
      // first chunk computed in registers first, a wave that reaches this barrier early has already
      // done that work (without WL the barrier sits at the end of the previous polynomial)
      if (WL) __syncthreads();
#pragma unroll
      for (int r = 0; r < NS1; ++r) {
        const uint32_t p0 = lpad(threadIdx.x + 256u * r);
#pragma unroll
        for (int m = 0; m < M1; ++m) sm[p0 + lofs<(1 << D1)>(m)] = x[r][m];
      }
      __syncthreads();
      fwd_chunk_ct<BL, BL - 1 - K1, K2, NR>(tws, q, n8q, lds_ld, [&](int, uint32_t, uint32_t pj0, auto& y) {
#pragma unroll
        for (int m = 0; m < (1 << K2); ++m) sm[pj0 + lofs<(1 << (BL - K1 - K2))>(m)] = y[m];
      });
      mid_sync();
      fwd_chunk_ct<BL, BL - 1 - K1 - K2, K3, NR>(tws, q, n8q, lds_ld, [&](int, uint32_t, uint32_t pj0, auto& y) {
#pragma unroll
        for (int m = 0; m < (1 << K3); ++m) sm[pj0 + lofs<(1 << (BL - K1 - K2 - K3))>(m)] = y[m];
      });
      mid_sync();
#pragma unroll
      for (int r = 0; r < NSL; ++r) {
        const uint32_t g = last_g(r), j0 = g << K4, pj0 = lpad(j0);
        uint64_t y[ML];
#pragma unroll
        for (int m = 0; m < ML; ++m) y[m] = sm[pj0 + m];
        fwd_set_ct<BL, K4 - 1, K4, NR>(y, g, tws, q, n8q);
        if (poly == 0) {  // NTT(v), lazy (< 12q): only ever a Shoup multiplicand
#pragma unroll
          for (int m = 0; m < ML; ++m) V[r][m] = y[m];
        } else {  // poly 1: c0 = v*b + (m + e0); poly 2: c1 = v*a + e1
          uint64_t* __restrict__ dst = ct + ((uint64_t)k * 2 + (poly - 1)) * LN + off + j0;
#pragma unroll
          for (int m = 0; m < ML; m += 2) {
            ulonglong2 c;
            c.x = red_any(shoup_lazy(V[r][m], P[r][m / 2].x, Ps[r][m / 2].x, q) + y[m], cst);
            c.y = red_any(shoup_lazy(V[r][m + 1], P[r][m / 2].y, Ps[r][m / 2].y, q) + y[m + 1], cst);
            *reinterpret_cast<ulonglong2*>(dst + m) = c;
          }
        }
      }
      if (!WL) __syncthreads();  // LDS is refilled by the next polynomial
    }
  }
}

constexpr uint64_t kEncNoredMinK = 192;  // launch_encrypt: the NORED tower split from this many ciphertexts
// enc_cols_fused's tower-split form up to this many ciphertexts per call: K = 4 21.1 vs 24.6 us/ct,
// K = 16 6.7 vs 7.3, but K = 64 4.1 vs 3.3 and K = 714 3.5 vs 2.6 (profiles/r04u/ts_k*.txt)
constexpr uint64_t kEncTsMaxK = 24;

size_t encrypt_scratch_bytes(const Params& p, uint64_t K) {
  // FFT buffer | pbuf [K][3][L][N] | me0 [K][N] int64 | ve [K][N] int16 | the large-value path's
  // per-ciphertext max, exponent and 2^logApprox mod q_t (launch_encrypt_approx)
  return K * (uint64_t)p.batch * sizeof(double2) + K * 3ull * p.L * p.N * sizeof(uint64_t) +
         K * (uint64_t)p.N * (sizeof(int64_t) + sizeof(int16_t)) + K * (8 + 8 + 16ull * p.L) + 64;
}

// encode's FFTSpecialInv of K slot vectors (x: n doubles, zero-padded) into fbuf [K][S] (complex); p.pack
// picks the kernels that read x: one value per slot, or an interleaved (re, im) pair (the _cx entry points)
void launch_encode_fft(const Params& p, const DeviceTables& dt, const double* x, uint64_t n, uint64_t K,
                       double2* fbuf, hipStream_t s) {
  const uint32_t logS = __builtin_ctz(p.batch);
  const uint32_t blkLog = fft_block_log(logS);
  const int logR = (int)(logS - blkLog);
  const size_t lds = sizeof(double2) << blkLog;
  const bool cx = p.pack != 0;
  if (logS == kFftWholeLogS && K >= kFftWholeMinK && switches().fft_whole) {  // a workgroup per vector
    hipLaunchKernelGGL(cx ? fft_inv_whole_cx : fft_inv_whole, dim3((uint32_t)K), dim3(1024), 0, s, x, n, fbuf,
                       dt.fft_inv);
  } else if (logR > 0) {
    const uint64_t nb = K * ((p.batch >> logR) / 256);
    if (cx) {
      FFT_DISPATCH(logR, fft_inv_cols_cx, dim3((uint32_t)nb), dim3(256), 0, s, x, n, fbuf, logS, dt.fft_inv);
    } else {
      FFT_DISPATCH(logR, fft_inv_cols, dim3((uint32_t)nb), dim3(256), 0, s, x, n, fbuf, logS,
                   dt.fft_inv);
    }
    const bool fct = switches().fft_ct;
    if (fct && blkLog == 10)
      hipLaunchKernelGGL((fft_inv_blocks_ct<10, 3, 3, 2, 2>), dim3((uint32_t)(K << logR)), dim3(128), 0, s, fbuf,
                         logS, dt.fft_inv);
    else if (fct && blkLog == 11)
      hipLaunchKernelGGL((fft_inv_blocks_ct<11, 3, 3, 3, 2>), dim3((uint32_t)(K << logR)), dim3(256), 0, s, fbuf,
                         logS, dt.fft_inv);
    else
      hipLaunchKernelGGL(fft_inv_blocks, dim3((uint32_t)(K << logR)), dim3(256), lds, s, x, n, fbuf,
                         logS, blkLog, 0, dt.fft_inv);
  } else {
    hipLaunchKernelGGL(cx ? fft_inv_blocks_cx : fft_inv_blocks, dim3((uint32_t)K), dim3(256), lds, s, x, n, fbuf,
                       logS, blkLog, 1, dt.fft_inv);
  }
  SHELFI_HIP(hipGetLastError());
}

void launch_encrypt(const Params& p, const DeviceTables& dt, const DeviceKeys& dk, const double* x,
                    uint64_t n, uint64_t K, uint64_t* ct, void* scratch, const uint32_t key[8],
                    uint64_t g0, GenFlag flag, hipStream_t s) {
  if (!K) return;
  const uint32_t logS = __builtin_ctz(p.batch);
  double2* fbuf = reinterpret_cast<double2*>(scratch);
  uint64_t* pbuf = reinterpret_cast<uint64_t*>(fbuf + K * (uint64_t)p.batch);
  // 1. FFTSpecialInv of each ciphertext's slot vector
  launch_encode_fft(p, dt, x, n, K, fbuf, s);
  Key8 k8;
  for (int i = 0; i < 8; ++i) k8.k[i] = key[i];
  const Switches& sw = switches();
  const uint32_t nblkLog = ntt_block_log(p.logN);
  const int nlogR = (int)(p.logN - nblkLog);
  // nlogR = 5 (2^16 over 2^11 blocks, 2^17): the 16-row kernel with the exchanged fifth stage (X5)
  const bool fused = (nlogR == 3 || nlogR == 4 || (nlogR == 5 && sw.enc_tab && sw.enc_x5)) && dt.enc_tab &&
                     sw.enc_fused;
  int64_t* me0 = reinterpret_cast<int64_t*>(pbuf + K * 3ull * p.L * p.N);
  int16_t* ve = reinterpret_cast<int16_t*>(me0 + K * (uint64_t)p.N);
  // NORED towers (fwd_set_ct): q < kNoRedQ, run unreduced through both passes — only with the
  // persistent blocks pass, and only as a suffix of the chain (q_0 the 60-bit tower, the rest
  // near 2^scale_bits); t_split = L turns it off
  const bool pp = fused && nblkLog == 11 && dt.red_ok && sw.enc_pp;
  uint32_t t_split = 0;
  while (t_split < p.L && p.q[t_split] >= kNoRedQ) ++t_split;
  for (uint32_t t = t_split; t < p.L; ++t)
    if (p.q[t] >= kNoRedQ) t_split = p.L;
  // the two tower classes take one blocks-pass launch each, in series; below kEncNoredMinK ciphertexts a
  // call is latency-bound and one launch over every tower (all reduced) is faster: K = 4 / 16 / 64 / 128
  // encrypt 18.7 / 6.5 / 3.67 / 3.23 vs 21.2 / 6.9 / 3.76 / 3.28 us/ct, K = 256 2.92 vs 2.88
  // (profiles/r05zc/nored_k.txt; tests/test_gpu_switches.py checks both paths bit for bit at K = 200)
  // At 2^16 (nlogR = 5, X5 columns) the split is slower at every K measured: K = 256 / 512 encrypt 8.91 / 8.50
  // us/ct in one reduced launch vs 9.00 / 8.74 split, while 2^15 K = 714 gains 2.75 vs 2.88 (profiles/r06f/nr_*)
  if (!pp || !sw.enc_nored || K < kEncNoredMinK || nlogR == 5) t_split = p.L;
  bool vt = false;  // NTT(v)'s columns pass as enc_vtab sums in the blocks pass (round 5)
  if (fused) {
    // 2+3a. encode + sampling + columns pass of v, m + e0, e1 for every tower
    const uint64_t nb = (K << (p.logN - (nlogR == 5 ? 4 : nlogR))) / 256;
    const bool tab = sw.enc_tab;
    // LDS column twiddles at 3 waves/SIMD with the tables (no SGPR / VGPR spills): enc_cols_fused 578 ->
    // 534 us per 714 cts (probes/r03_enc_cols_twl.txt; the scalar-loaded form was removed in round 5)
#define ENC_COLS(GRID, ...)                                                                                     \
  hipLaunchKernelGGL((enc_cols_fused<__VA_ARGS__>), dim3((uint32_t)(GRID)), dim3(256), 0, s, fbuf, K, p.logN, logS, p.L, \
                     p.delta, dt.cdt, dt.cdt_len, k8, g0, dt.tc, dt.psi_rev, dt.psi_rev_sh, pbuf, flag, t_split,    \
                     dt.enc_tab)
    // small calls (K <= kEncTsMaxK at 4 towers): one wave per tower (TS), so a call of a few
    // ciphertexts spreads over 4x the waves; SHELFI_ENC_TS=0 / 1 forces either (A/B switch)
    const bool ts = nlogR == 4 && tab && p.L == 4 && (sw.enc_ts >= 0 ? sw.enc_ts == 1 : K <= kEncTsMaxK);
    vt = pp && tab && !ts && nlogR == 4 && dt.enc_vtab && sw.enc_vt && ntt_wave_local();
    // X5: 16 register rows + the exchanged fifth stage (10 VGPRs spilled at 3 waves / SIMD; the
    // spill-free 2-wave build ran 3-4% slower, profiles/r06b)
    if (nlogR == 5)
      ENC_COLS(nb, 4, true, 3, true, false, false, true);
    else if (vt)  // v's columns pass left to the blocks pass (enc_vtab sums)
      ENC_COLS(nb, 4, true, 3, true, false, true);
    else if (ts)  // 64 columns per workgroup
      ENC_COLS(nb * 4, 4, true, 3, true, true);
    else if (nlogR == 3 && tab)
      ENC_COLS(nb, 3, true);
    else if (nlogR == 3)
      ENC_COLS(nb, 3, false);
    else if (tab)  // 164 VGPRs without spills at 3 waves (4 would spill 36)
      ENC_COLS(nb, 4, true, 3, true);
    else
      ENC_COLS(nb, 4, false);
#undef ENC_COLS
    SHELFI_HIP(hipGetLastError());
  } else {
    // 2. encode (scale/round) + sampling -> compact record
    const uint64_t threads = K * (p.N / 16);  // one per v2 sample group
    hipLaunchKernelGGL(enc_prep_kernel, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, s, fbuf,
                       K, p.logN, logS, p.delta, dt.cdt, dt.cdt_len, k8, g0, me0, ve, flag);
    SHELFI_HIP(hipGetLastError());
  }
  // 3. NTT of v, m + e0, e1 per tower (columns pass expands the record), then the
  // blocks pass fused with the public-key combine writes the ciphertexts
  if (nlogR > 0 && !fused) {
    const uint64_t nb = K * ((p.N >> nlogR) / 256);
#define COLS_ENC1(LR, POLY)                                                                               \
  hipLaunchKernelGGL((ntt_fwd_cols_enc<LR, POLY>), dim3((uint32_t)nb), dim3(256), 0, s, me0, ve, K, p.logN, p.L, \
                     dt.tc, dt.psi_rev, dt.psi_rev_sh, pbuf);
#define COLS_ENC(LR) COLS_ENC1(LR, 0) COLS_ENC1(LR, 1) COLS_ENC1(LR, 2)
    switch (nlogR) {
      case 1: COLS_ENC(1) break;
      case 2: COLS_ENC(2) break;
      case 3: COLS_ENC(3) break;
      case 4: COLS_ENC(4) break;
      case 5: COLS_ENC(5) break;
      case 6: COLS_ENC(6) break;
      default: throw Error{SHELFI_ERR_ARG, "unsupported ring dimension"};
    }
#undef COLS_ENC
#undef COLS_ENC1
    SHELFI_HIP(hipGetLastError());
  }
  const uint64_t nbb = K * p.L << nlogR;
  if (nbb > 0x7FFFFFFFull) throw Error{SHELFI_ERR_ARG, "encrypt batch too large"};
  const uint32_t xg = xcd_combos(p.L << nlogR);
  if (pp) {  // one launch per tower class, each spread over all CUs
    const bool wl = ntt_wave_local();
    const auto launch_pp = [&](uint32_t ta, uint32_t nt, bool nr) {
      const uint32_t ncombo = nt << nlogR;
      const uint32_t pc = pp_per_combo(ncombo, K, 3);
#define ENC_PP(NR, WL, VT)                                                                                       \
  hipLaunchKernelGGL((ntt_fwd_blocks_enc_pp<11, 3, 3, 3, 2, NR, WL, VT>), dim3(ncombo * pc), dim3(256), 0, s, pbuf, \
                     p.L, p.logN, dt.tw_fwd_blk, dt.tc, dk.pk, dk.pk_sh, ct, (uint32_t)K, pc, ta, nt, dt.enc_vtab)
      if (nr && wl && vt) ENC_PP(true, true, true);
      else if (nr && wl) ENC_PP(true, true, false);
      else if (nr) ENC_PP(true, false, false);
      else if (wl && vt) ENC_PP(false, true, true);
      else if (wl) ENC_PP(false, true, false);
      else ENC_PP(false, false, false);
#undef ENC_PP
    };
    if (t_split > 0) launch_pp(0u, t_split, false);
    if (t_split < p.L) launch_pp(t_split, p.L - t_split, true);
  } else if (nlogR > 0 && nblkLog == 11 && dt.red_ok)
    hipLaunchKernelGGL((ntt_fwd_blocks_enc_ct<11, 3, 3, 3, 2>), dim3((uint32_t)nbb), dim3(256), 0, s,
                       pbuf, p.L, p.logN, dt.tw_fwd_blk, dt.tc, dk.pk, dk.pk_sh, ct, 0u, xg);
  else if (nlogR > 0 && nblkLog == 12 && dt.red_ok)
    hipLaunchKernelGGL((ntt_fwd_blocks_enc_ct<12, 3, 3, 3, 3>), dim3((uint32_t)nbb), dim3(256), 0, s,
                       pbuf, p.L, p.logN, dt.tw_fwd_blk, dt.tc, dk.pk, dk.pk_sh, ct, 0u, xg);
  else {
#define ENC_BLOCKS(PP)                                                                                          \
  hipLaunchKernelGGL(ntt_fwd_blocks_enc<PP>, dim3((uint32_t)nbb), dim3(256), sizeof(uint64_t) << nblkLog, s, pbuf, \
                     p.L, p.logN, (uint32_t)nlogR, dt.psi_rev, dt.psi_rev_sh, dt.tc, dk.pk, dk.pk_sh, ct,        \
                     nlogR > 0 ? (const int64_t*)nullptr : me0, nlogR > 0 ? (const int16_t*)nullptr : ve)
    if (nblkLog > 11) ENC_BLOCKS(8);
    else ENC_BLOCKS(4);
#undef ENC_BLOCKS
  }
  SHELFI_HIP(hipGetLastError());
}

// ---------------------------------------------- encode's large-value path ----
// PALISADE 1.11 CKKSPackedEncoding::Encode (ckks.cpp:80) scales a slot vector down before rounding when
// its largest coefficient would not fit a 62-bit word [PALISADE-1.11, restated in
// oracle/ckks_oracle.c or_encode_coeffs_ex; parity with PALISADE unpinned]:
//   logc = max over nonzero v_i = FFTSpecialInv(x)_i * Delta of ceil(log2 |v_i|);
//   logApprox = max(0, logc - 62); r_i = llround(v_i / 2^logApprox), wrapped as FitToNativeVector
//   does with Max64BitValue() = 2^63 - 513 (enc_fit_wrap); residue_t = r_i * 2^logApprox mod q_t.
// The fast encrypt kernels handle |v| <= 2^61 (logApprox = 0, no wrap) and flag anything larger;
// the call is then redone here: per-ciphertext max |v| on the device, logApprox from glibc's log2 on
// the host (the function PALISADE calls; one exponent per ciphertext), then the coefficients,
// samples and the 2^logApprox factor written as canonical residues [K][3][L][N], the generic NTT,
// and the public-key combine.  Same ChaCha20 streams as the fast path, so only the message
// coefficients can differ, and only where the fast path refused.
__device__ __forceinline__ int64_t enc_fit_wrap(int64_t r) {
  constexpr int64_t kMax64 = 9223372036854775295LL;  // PALISADE Max64BitValue(): 2^63 - 513
  constexpr int64_t hf = kMax64 >> 1;
  if (r > hf) return r - kMax64;
  if (r < 0 && kMax64 + r <= hf) return r + kMax64;
  return r;
}

// per ciphertext: max |Re|, |Im| of its FFTSpecialInv output, as the bits of a positive double
__global__ __launch_bounds__(256) void enc_maxabs_kernel(const double2* __restrict__ fbuf, uint32_t logS,
                                                         uint64_t* __restrict__ amax) {
  const uint32_t S = 1u << logS;
  const double2* __restrict__ f = fbuf + (uint64_t)blockIdx.x * S;
  uint64_t m = 0;
  for (uint32_t i = threadIdx.x; i < S; i += 256) {
    const double2 v = f[i];
    const uint64_t a = (uint64_t)__double_as_longlong(fabs(v.x)), b = (uint64_t)__double_as_longlong(fabs(v.y));
    m = max(m, max(a, b));
  }
  __shared__ uint64_t red[256];
  red[threadIdx.x] = m;
  __syncthreads();
  for (uint32_t w = 128; w; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] = max(red[threadIdx.x], red[threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x == 0) amax[blockIdx.x] = red[0];
}

// thread = sample group h of ciphertext k (enc_prep_kernel's mapping and streams): v, m + e0, e1 as
// canonical residues of every tower into pbuf [K][3][L][N] (COEFFICIENT domain)
__global__ __launch_bounds__(256) void enc_expand_approx_kernel(
    const double2* __restrict__ fbuf, uint64_t K, uint32_t logN, uint32_t logS, uint32_t L, double delta,
    const uint64_t* __restrict__ cdt, int T, Key8 key, uint64_t g0, const TowerConst* __restrict__ tcs,
    const int32_t* __restrict__ log_approx, const uint64_t* __restrict__ pw, uint64_t* __restrict__ pbuf) {
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
  const double approx = ldexp(1.0, log_approx[k]);
  uint32_t w[16];
  chacha20_block32(key, h >> 2, nonce, w);
  uint32_t u[4] = {w[4 * (h & 3)], w[4 * (h & 3) + 1], w[4 * (h & 3) + 2], w[4 * (h & 3) + 3]};
  int32_t vv[16], e0[16], e1[16];
  int64_t mm[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) vv[i] = (int32_t)trit_next(u) - 1;
  chacha20_block32(key, V0 + h, nonce, w);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint32_t j = h + N16 * i;
    const uint32_t jj = j < half ? j : j - half;
    int64_t m = 0;
    if ((jj & ((1u << gapLog) - 1)) == 0) {
      const double2 cv = fbuf[k * S + bitrev_dev(jj >> gapLog, logS)];
      const double val = __dmul_rn(__ddiv_rn(j < half ? cv.x : cv.y, dS), delta);
      m = enc_fit_wrap(round_half_away(__ddiv_rn(val, approx)));
    }
    mm[i] = m;
    e0[i] = (int32_t)gauss32(w[i], thi, tlo, [&] { return chacha20_word(key, V0 + 2 * N16 + h, nonce, i); });
  }
  chacha20_block32(key, V0 + N16 + h, nonce, w);
#pragma unroll
  for (int i = 0; i < 16; ++i)
    e1[i] = (int32_t)gauss32(w[i], thi, tlo, [&] { return chacha20_word(key, V0 + 3 * N16 + h, nonce, i); });
  const uint64_t LN = (uint64_t)L << logN;
  for (uint32_t t = 0; t < L; ++t) {
    const TowerConst cst = tcs[t];
    const uint64_t q = cst.q, P = pw[(k * L + t) * 2], Psh = pw[(k * L + t) * 2 + 1];
    uint64_t* __restrict__ o = pbuf + k * 3 * LN + ((uint64_t)t << logN) + h;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint64_t j = (uint64_t)N16 * i;
      o[j] = small_mod(vv[i], q);
      o[LN + j] = addmod(shoup_mul(mod_signed_dev(mm[i], cst), P, Psh, q), small_mod(e0[i], q), q);
      o[2 * LN + j] = small_mod(e1[i], q);
    }
  }
}

// c0 = NTT(v) b + NTT(m + e0), c1 = NTT(v) a + NTT(e1) from canonical EVALUATION residues
__global__ __launch_bounds__(256) void enc_combine_kernel(const uint64_t* __restrict__ pbuf, uint64_t K,
                                                          uint32_t logN, uint32_t L,
                                                          const TowerConst* __restrict__ tcs,
                                                          const uint64_t* __restrict__ pk,
                                                          const uint64_t* __restrict__ pk_sh,
                                                          uint64_t* __restrict__ ct) {
  const uint64_t LN = (uint64_t)L << logN;
  const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= K * LN) return;
  const uint64_t k = gid / LN, r = gid - k * LN;
  const uint64_t q = tcs[r >> logN].q;
  const uint64_t* __restrict__ b = pbuf + k * 3 * LN;
  const uint64_t V = b[r], M = b[LN + r], E = b[2 * LN + r];
  ct[k * 2 * LN + r] = addmod(shoup_mul(V, pk[r], pk_sh[r], q), M, q);
  ct[k * 2 * LN + LN + r] = addmod(shoup_mul(V, pk[LN + r], pk_sh[LN + r], q), E, q);
}

static uint64_t host_powmod2(uint32_t e, uint64_t q) {
  unsigned __int128 r = 1 % q, b = 2 % q;
  for (; e; e >>= 1) {
    if (e & 1) r = r * b % q;
    b = b * b % q;
  }
  return (uint64_t)r;
}

void launch_encrypt_approx(const Params& p, const DeviceTables& dt, const DeviceKeys& dk, const double* x,
                           uint64_t n, uint64_t K, uint64_t* ct, void* scratch, const uint32_t key[8],
                           uint64_t g0, hipStream_t s) {
  if (!K) return;
  const uint32_t logS = __builtin_ctz(p.batch);
  double2* fbuf = reinterpret_cast<double2*>(scratch);
  uint64_t* pbuf = reinterpret_cast<uint64_t*>(fbuf + K * (uint64_t)p.batch);
  // aux region after me0 / ve (encrypt_scratch_bytes): amax [K] u64 | log_approx [K] i32 (8-aligned) |
  // pw [K][L][2] u64
  uint8_t* aux = reinterpret_cast<uint8_t*>(pbuf + K * 3ull * p.L * p.N) + K * (uint64_t)p.N * 10;
  uint64_t* amax = reinterpret_cast<uint64_t*>(aux);
  int32_t* la_dev = reinterpret_cast<int32_t*>(amax + K);
  uint64_t* pw_dev = amax + K + (K + 1) / 2;
  launch_encode_fft(p, dt, x, n, K, fbuf, s);
  hipLaunchKernelGGL(enc_maxabs_kernel, dim3((uint32_t)K), dim3(256), 0, s, fbuf, logS, amax);
  SHELFI_HIP(hipGetLastError());
  std::vector<uint64_t> hm(K);
  SHELFI_HIP(hipMemcpyAsync(hm.data(), amax, K * 8, hipMemcpyDeviceToHost, s));
  SHELFI_HIP(hipStreamSynchronize(s));
  std::vector<int32_t> la(K);
  std::vector<uint64_t> pw(K * p.L * 2);
  for (uint64_t k = 0; k < K; ++k) {
    double M;
    std::memcpy(&M, &hm[k], 8);
    const double v = (M / (double)p.batch) * p.delta;  // the kernels' (c / S) * Delta, monotone in c
    int logc = 0;
    if (v != 0) logc = std::max(0, (int)std::ceil(std::log2(v)));  // glibc, as Encode calls it
    la[k] = logc > 62 ? logc - 62 : 0;
    for (uint32_t t = 0; t < p.L; ++t) {
      const uint64_t q = p.q[t], w = host_powmod2((uint32_t)la[k], q);
      pw[(k * p.L + t) * 2] = w;
      pw[(k * p.L + t) * 2 + 1] = (uint64_t)(((unsigned __int128)w << 64) / q);
    }
  }
  SHELFI_HIP(hipMemcpyAsync(la_dev, la.data(), K * 4, hipMemcpyHostToDevice, s));
  SHELFI_HIP(hipMemcpyAsync(pw_dev, pw.data(), pw.size() * 8, hipMemcpyHostToDevice, s));
  Key8 k8;
  for (int i = 0; i < 8; ++i) k8.k[i] = key[i];
  const uint64_t threads = K * (p.N / 16);
  hipLaunchKernelGGL(enc_expand_approx_kernel, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, s, fbuf, K,
                     p.logN, logS, p.L, p.delta, dt.cdt, dt.cdt_len, k8, g0, dt.tc, la_dev, pw_dev, pbuf);
  SHELFI_HIP(hipGetLastError());
  launch_ntt(pbuf, K * 3ull * p.L, p.L, p.logN, false, dt, s);
  const uint64_t tot = K * (uint64_t)p.L * p.N;
  hipLaunchKernelGGL(enc_combine_kernel, dim3((uint32_t)((tot + 255) / 256)), dim3(256), 0, s, pbuf, K, p.logN, p.L,
                     dt.tc, dk.pk, dk.pk_sh, ct);
  SHELFI_HIP(hipGetLastError());
  SHELFI_HIP(hipStreamSynchronize(s));  // the host tables above are uploaded from pageable memory
}

}  // namespace shelfi
