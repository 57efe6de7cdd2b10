// decrypt.hip — decrypt + decode: c0 + c1*s, the inverse NTT, the centred CRT, PALISADE's decode
// noise flooding and FFTSpecial.
//
// Kernels (roofline class in DESIGN.md):
//   ntt_inv_blocks(_dec_ct, _dec_pp)  c0 + c1*s formed on load (ckks.cpp:189) + first INTT stages
//                      (their FuseIn forms: the threshold fusion's sum of partial decryptions instead,
//                      mkhe.cpp:402; the partial decryption itself is threshold.hip)
//   ntt_inv_cols_crt   last INTT stages fused with the exact centered CRT -> double / scale
//   crt_decode_kernel  the CRT alone (shapes the fused kernel does not cover)
//   decode_flood_kernel, decode_stats_kernel, flood_add_kernel  the decode noise
//   fft_fwd_*          CKKS special FFT (decode), 2 passes or one workgroup per vector
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <type_traits>

#include "dev_common.h"
#include "shelfi_internal.h"
#include "transform_dev.h"

namespace shelfi {

// Decrypt's first INTT pass at compile-time shape (chunks K1..K4, sum BL; needs
// logN > BL): c0 + c1*s is formed straight into the first chunk's registers from the
// ciphertext batch [K][2][L][N], and the last chunk writes the lazy ([0, 8q)) block to
// dbuf [K][L][N] from registers for ntt_inv_cols.  Same contract as ntt_inv_blocks with
// ct != nullptr and scale_ninv = 0.
// SUM: the ciphertexts are a collective's unfolded uint64 sums of <= 16 canonical residues
// (shelfi_dev_combine_arena with fold = 0): c0 is reduced on load (red_any, [0, 2q)), c1 needs
// nothing (the lazy Shoup product takes any 64-bit multiplicand) — the mod-q fold of the
// combine happens here instead of in a separate pass over the share.
// FZ = FuseIn (threshold fusion, mkhe.cpp:402): no ciphertext and no key -- the input is the sum of
// fz.P partial decryptions [K][ctL][N], added as uint64 words while they load (<= 16 canonical
// residues) and folded by the SUM reduction; the c1*s product is skipped.
template <int BL, int K1, int K2, int K3, int K4, bool SUM = false, class FZ = NoFuse>
__global__ __launch_bounds__(256) void ntt_inv_blocks_dec_ct(uint64_t* __restrict__ dbuf, uint32_t L,
                                                             uint32_t logN,
                                                             const ulonglong2* __restrict__ twb,
                                                             const TowerConst* __restrict__ tcs,
                                                             const uint64_t* __restrict__ ct,
                                                             const uint64_t* __restrict__ sk,
                                                             const uint64_t* __restrict__ sksh,
                                                             uint32_t xg, uint32_t ctL, FZ fz) {
  static_assert(K1 + K2 + K3 + K4 == BL, "chunk plan must cover the block");
  constexpr bool FUSE = std::is_same<FZ, FuseIn>::value;
  static_assert(!FUSE || SUM, "the fused partials are folded by the SUM reduction");
  __shared__ __attribute__((aligned(16))) uint64_t sm[lpad_size(BL)];
  const uint32_t sstart = logN - BL;
  const uint32_t bid = xcd_block(blockIdx.x, xg);
  const uint32_t b = bid & ((1u << sstart) - 1);
  const uint32_t poly = bid >> sstart;  // k * L + t
  const uint32_t t = poly % L, k = poly / L;
  const TowerConst& cst = tcs[t];
  const uint64_t q = cst.q, n4q = cst.n4q, n8q = cst.n8q;
  const ulonglong2* __restrict__ tb = twb + ((uint64_t)t << logN) + ((uint64_t)b << BL);
  const uint64_t off = ((uint64_t)t << logN) + ((uint64_t)b << BL);
  const uint64_t LN = (uint64_t)L << logN;
  const uint64_t CLN = (uint64_t)ctL << logN;  // the ciphertexts' towers (>= L, decode_towers)
  const uint64_t* __restrict__ c0 = ct + (uint64_t)k * 2 * CLN + off;
  const uint64_t* __restrict__ c1 = c0 + CLN;
  const uint64_t* __restrict__ s = sk + off;
  const uint64_t* __restrict__ ss = sksh + off;
  const auto lds_ld = [&](uint32_t, uint32_t pj) { return sm[pj]; };
  // first chunk: contiguous sets of 2^K1 (T0 = 0)
  inv_chunk_ct<BL, 0, K1, false>(tb, q, n8q,
                          [&](uint32_t j, uint32_t) {
                            if constexpr (FUSE) {
                              // the first two partials as independent loads (P = 2: no dependent chain)
                              const uint64_t e = (uint64_t)k * CLN + off + j;
                              uint64_t a = fz.part[0][e] + (fz.P > 1 ? fz.part[1][e] : 0);
                              for (uint32_t i = 2; i < fz.P; ++i) a += fz.part[i][e];
                              return red_any(a, cst);
                            } else {
                              const uint64_t a0 = SUM ? red_any(c0[j], cst) : c0[j];
                              return csub_neg(a0 + shoup_lazy(c1[j], s[j], ss[j], q), n4q);
                            }
                          },
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
  uint64_t* __restrict__ dst = dbuf + (uint64_t)k * LN + off;
  inv_chunk_ct<BL, BL - K4, K4, true>(tb, q, n8q, lds_ld, [&](int, uint32_t j0, uint32_t, auto& x) {
#pragma unroll
    for (int m = 0; m < (1 << K4); ++m) dst[j0 + (m << (BL - K4))] = x[m];
  });
}

// Persistent, software-pipelined form of ntt_inv_blocks_dec_ct (round 3).  The one-shot
// kernel loads its whole first chunk from HBM and only then computes, and all its workgroups
// start together: measured 0.48 of the VALU issue peak and ~3.6 TB/s, neither bound reached.
// Here a workgroup owns one (tower, block) combo and walks ciphertexts k0, k0 + P, ...:
//  * the combo's 2^BL twiddle pairs are copied into LDS once (32 KiB), so the per-chunk
//    twiddle reads leave the vector-memory queue (whose in-order vmcnt would otherwise make
//    every twiddle wait drain the prefetch below);
//  * the secret-key words s, s' of the first chunk's elements stay in registers;
//  * ciphertext k + P's c0 / c1 words are loaded into registers right after ciphertext k's
//    have been consumed, so their HBM latency hides behind k's stages.
// Same arithmetic, same lazy bounds and same dbuf contents as ntt_inv_blocks_dec_ct.
// WL: as ntt_fwd_blocks_enc_pp's, mirrored: the first three chunks (half-sizes 1 .. 2^(BL-K4-1))
// stay inside 512-element sub-blocks, each wave's own once the first chunk's sets are dealt as
// g = 2 * 64 w + 64 r + lane; only the exchange into the last chunk crosses waves.
// FZ = FuseIn: as ntt_inv_blocks_dec_ct's.  No key words are held; the prefetch issues partials 0 and 1 of
// the next ciphertext as it issues c0 and c1 (added when consumed) and sums partials 2 .. P-1 itself.
template <int BL, int K1, int K2, int K3, int K4, bool SUM = false, bool WL = false, class FZ = NoFuse>
__global__ __launch_bounds__(256) void ntt_inv_blocks_dec_pp(uint64_t* __restrict__ dbuf, uint32_t L,
                                                             uint32_t logN,
                                                             const ulonglong2* __restrict__ twb,
                                                             const TowerConst* __restrict__ tcs,
                                                             const uint64_t* __restrict__ ct,
                                                             const uint64_t* __restrict__ sk,
                                                             const uint64_t* __restrict__ sksh, uint32_t K,
                                                             uint32_t per_combo, uint32_t ctL, FZ fz) {
  static_assert(K1 + K2 + K3 + K4 == BL, "chunk plan must cover the block");
  constexpr bool FUSE = std::is_same<FZ, FuseIn>::value;
  static_assert(!FUSE || SUM, "the fused partials are folded by the SUM reduction");
  constexpr int M1 = 1 << K1, NS1 = (1 << (BL - K1)) / 256;
  static_assert(!WL || (BL == 11 && K1 == 2 && K2 == 3 && K3 == 3 && K4 == 3), "wave-local plan");
  __shared__ __attribute__((aligned(16))) ulonglong2 tws[1 << BL];
  __shared__ __attribute__((aligned(16))) uint64_t sm[lpad_size(BL)];
  // the first chunk's set r of this thread (its elements g 2^K1 + m)
  const auto first_g = [&](int r) -> uint32_t {
    return WL ? ((threadIdx.x >> 6) * (64u * NS1) + 64u * r + (threadIdx.x & 63u)) : threadIdx.x + 256u * r;
  };
  const uint32_t sstart = logN - BL;
  const uint32_t ncombo = L << sstart;
  const uint32_t combo = blockIdx.x % ncombo;
  const uint32_t b = combo & ((1u << sstart) - 1), t = combo >> sstart;
  const TowerConst& cst = tcs[t];
  const uint64_t q = cst.q, n4q = cst.n4q, n8q = cst.n8q;
  const uint64_t off = ((uint64_t)t << logN) + ((uint64_t)b << BL);
  const uint64_t LN = (uint64_t)L << logN;
  {
    const ulonglong2* __restrict__ src = twb + off;
    for (uint32_t i = threadIdx.x; i < (1u << BL); i += 256) tws[i] = src[i];
  }
  // first chunk (T0 = 0): set r of this thread = elements (tid + 256 r) 2^K1 + m
  uint64_t sv[NS1][M1], sw[NS1][M1], p0[NS1][M1], p1[NS1][M1];
  uint64_t p2[FUSE ? NS1 : 1][FUSE ? M1 : 1];  // FUSE: the sum of partials 2 .. P-1
  if constexpr (!FUSE) {
#pragma unroll
    for (int r = 0; r < NS1; ++r)
#pragma unroll
      for (int m = 0; m < M1; ++m) {
        const uint32_t j = (first_g(r) << K1) + m;
        sv[r][m] = sk[off + j];
        sw[r][m] = sksh[off + j];
      }
  }
  uint32_t k = blockIdx.x / ncombo;
  const uint64_t CLN = (uint64_t)ctL << logN;  // the ciphertexts' towers (>= L, decode_towers)
  const auto fetch = [&](uint32_t kk) {
    if constexpr (FUSE) {
      // partials 2 .. P-1 are summed here, two loads in flight per element (their waits sit in the
      // prefetch); partials 0 and 1 are then only issued, like c0 and c1, and land while the previous
      // ciphertext is transformed -- P = 2 waits for nothing here
      const uint64_t eoff = (uint64_t)kk * CLN + off;
#pragma unroll
      for (int r = 0; r < NS1; ++r)
#pragma unroll
        for (int m = 0; m < M1; ++m) p2[r][m] = 0;
      uint32_t i = 2;
      for (; i + 1 < fz.P; i += 2) {
        const uint64_t* __restrict__ pa = fz.part[i] + eoff;
        const uint64_t* __restrict__ pb = fz.part[i + 1] + eoff;
        uint64_t ta[NS1][M1], tb[NS1][M1];
#pragma unroll
        for (int r = 0; r < NS1; ++r)
#pragma unroll
          for (int m = 0; m < M1; ++m) {
            const uint32_t j = (first_g(r) << K1) + m;
            ta[r][m] = __builtin_nontemporal_load(pa + j);
            tb[r][m] = __builtin_nontemporal_load(pb + j);
          }
#pragma unroll
        for (int r = 0; r < NS1; ++r)
#pragma unroll
          for (int m = 0; m < M1; ++m) p2[r][m] += ta[r][m] + tb[r][m];
      }
      if (i < fz.P) {
        const uint64_t* __restrict__ pa = fz.part[i] + eoff;
#pragma unroll
        for (int r = 0; r < NS1; ++r)
#pragma unroll
          for (int m = 0; m < M1; ++m) p2[r][m] += __builtin_nontemporal_load(pa + ((first_g(r) << K1) + m));
      }
      const uint64_t* __restrict__ q0 = fz.part[0] + eoff;
      const uint64_t* __restrict__ q1 = fz.part[fz.P > 1 ? 1 : 0] + eoff;
#pragma unroll
      for (int r = 0; r < NS1; ++r)
#pragma unroll
        for (int m = 0; m < M1; ++m) {
          const uint32_t j = (first_g(r) << K1) + m;
          p0[r][m] = __builtin_nontemporal_load(q0 + j);
          p1[r][m] = __builtin_nontemporal_load(q1 + j);
        }
    } else {
      const uint64_t* __restrict__ c0 = ct + (uint64_t)kk * 2 * CLN + off;
#pragma unroll
      for (int r = 0; r < NS1; ++r)
#pragma unroll
        for (int m = 0; m < M1; ++m) {
          const uint32_t j = (first_g(r) << K1) + m;
          p0[r][m] = __builtin_nontemporal_load(c0 + j);
          p1[r][m] = __builtin_nontemporal_load(c0 + CLN + j);
        }
    }
  };
  if (k < K) fetch(k);
  __syncthreads();  // the twiddle slice is in LDS
  const auto lds_ld = [&](uint32_t, uint32_t pj) { return sm[pj]; };
#pragma unroll 1
  for (; k < K; k += per_combo) {
    uint64_t x[NS1][M1];
#pragma unroll
    for (int r = 0; r < NS1; ++r)
#pragma unroll
      for (int m = 0; m < M1; ++m) {
        if constexpr (FUSE) {
          x[r][m] = red_any(p0[r][m] + (fz.P > 1 ? p1[r][m] : 0) + p2[r][m], cst);
        } else {
          const uint64_t a0 = SUM ? red_any(p0[r][m], cst) : p0[r][m];
          x[r][m] = csub_neg(a0 + shoup_lazy(p1[r][m], sv[r][m], sw[r][m], q), n4q);
        }
      }
    if (k + per_combo < K) fetch(k + per_combo);  // lands while this ciphertext is transformed
#pragma unroll
    for (int r = 0; r < NS1; ++r) {  // first chunk: stages i < K1 of the contiguous sets
      const uint32_t g = first_g(r);
#pragma unroll
      for (int i = 0; i < K1; ++i) {
        const int hm = 1 << i;
        const ulonglong2* tw = tws + (1u << (BL - 1 - i)) + (g << (K1 - 1 - i));
#pragma unroll
        for (int gs = 0; gs < (M1 >> (i + 1)); ++gs) {
          const ulonglong2 W = tw[gs];
#pragma unroll
          for (int mm = 0; mm < hm; ++mm) {
            if (gs_in8<false>(i, mm))
              gs_bfly_b<true>(x[r][gs * 2 * hm + mm], x[r][gs * 2 * hm + mm + hm], W.x, W.y, q, n8q);
            else
              gs_bfly_b<false>(x[r][gs * 2 * hm + mm], x[r][gs * 2 * hm + mm + hm], W.x, W.y, q, n8q);
          }
        }
      }
      if (!WL) {
        const uint32_t pj0 = lpad(g << K1);
#pragma unroll
        for (int m = 0; m < M1; ++m) sm[pj0 + lofs<1>(m)] = x[r][m];
      }
    }
    if (WL) {
      // the previous ciphertext's last-chunk reads (every wave's) must be done before this wave
      // refills its sub-block; the first chunk above already ran in registers meanwhile
      __syncthreads();
#pragma unroll
      for (int r = 0; r < NS1; ++r) {
        const uint32_t pj0 = lpad(first_g(r) << K1);
#pragma unroll
        for (int m = 0; m < M1; ++m) sm[pj0 + lofs<1>(m)] = x[r][m];
      }
      wave_lds_sync();
    } else {
      __syncthreads();
    }
    inv_chunk_ct<BL, K1, K2, true>(tws, q, n8q, lds_ld, [&](int, uint32_t, uint32_t pj0, auto& y) {
#pragma unroll
      for (int m = 0; m < (1 << K2); ++m) sm[pj0 + lofs<(1 << K1)>(m)] = y[m];
    });
    if (WL)
      wave_lds_sync();
    else
      __syncthreads();
    inv_chunk_ct<BL, K1 + K2, K3, true>(tws, q, n8q, lds_ld, [&](int, uint32_t, uint32_t pj0, auto& y) {
#pragma unroll
      for (int m = 0; m < (1 << K3); ++m) sm[pj0 + lofs<(1 << (K1 + K2))>(m)] = y[m];
    });
    __syncthreads();
    uint64_t* __restrict__ dst = dbuf + (uint64_t)k * LN + off;
    inv_chunk_ct<BL, BL - K4, K4, true>(tws, q, n8q, lds_ld, [&](int, uint32_t j0, uint32_t, auto& y) {
#pragma unroll
      for (int m = 0; m < (1 << K4); ++m) dst[j0 + (m << (BL - K4))] = y[m];
    });
    if (!WL) __syncthreads();  // sm is rewritten by the next ciphertext's first chunk
  }
}

// One coefficient of the centred CRT over the decode's towers: y(t) in [0, q_t) are
// b_t (Q/q_t)^-1 mod q_t for the L <= 7 towers; X = sum_t y_t (Q/q_t) - k Q with k = round(sum_t
// y_t / q_t), then (double)X * (1/scale) (PALISADE Decode: ConvertToDouble * scalingFactorPre *
// 2^-p), X read as a signed 128-bit integer: (double)|X|_hi 2^64 + (double)|X|_lo with its sign
// (the oracle's or_mw_to_double restricted to two words).
//
// The sum runs in NC 30-bit limb columns (y_t = a + b 2^30; every column is a sum of <= 2L
// products below 2^60 plus k times a 30-bit limb, below 2^64 without carries: one v_mad_u64_u32
// per product), then one carry pass.  NC (DeviceTables::crt_nc) is chosen so that the columns
// hold X' = sum_t y_t (Q/q_t) - k Q exactly in two's complement (|X'| < L Q): whatever k's binary32
// estimate gave, X' is a representative of X mod Q, and it is the centred one exactly when it lies
// in (-2^127, 2^127) -- the value range of this path (round 6).  Bits 127 .. 30 NC - 1 of X' all
// equal is therefore the exact test of "this output is right": otherwise *wide is set and the
// caller redoes the call through crt_exact_kernel over every tower (any |X| <= (Q - 1) / 2, as
// PALISADE's BigInteger decode).  No X in the old range sets it: over the prefix decode_towers keeps
// (Q > 2^130), |X| < 2^127 puts sum_t y_t / q_t within 2^-3 of k, and the binary32 estimate errs by
// at most ~L 2^-21 (terms (y_t >> s_t) * (2^s_t / q_t), y_t >> s_t < 2^32, TowerConst::crt_sh), so
// k is exact and the output bits are the round-5 ones.
//
// EDGE (DeviceTables::crt_edge): a chain at or below 2^130 is decoded whole, and there that argument
// fails near +-Q/2: sum_t y_t / q_t = k + X / Q lies within the estimate's error of the rounding
// boundary k +- 1/2, a k that is off by one gives X' = X -+ Q, and with Q/2 < 2^127 that wrong X' is
// inside the 128-bit range.  The estimate errs by less than 2^-18 for L <= 7 (each term's three
// binary32 roundings, 3 x 2^-24 of a term below 1; each running sum's, half an ulp of a value below
// 8, 2^-22; the + 0.5's), so k can be wrong only when |X| > Q/2 - Q 2^-18, and then |X'| >= Q/2 as
// well.  Flagging every |X'| >= (Q - 1) / 2 - floor(Q 2^-16) (TowerConst::crt_edge, 4x that bound)
// therefore catches every wrong output; the right ones in that band are merely redone exactly.  Not
// instantiated for prefixes above 2^130, whose code is unchanged.
template <int NC, bool EDGE = false, class YF>
__device__ __forceinline__ double crt_value(YF yf, uint32_t L, const TowerConst* __restrict__ tcs,
                                            double inv_scale, bool& wide) {
  static_assert(NC >= 5 && NC <= 7, "crt columns");
  constexpr uint32_t M30 = (1u << 30) - 1;
  uint64_t sc[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) sc[j] = 0;
  float f = 0.f;
#pragma unroll 1
  for (uint32_t t = 0; t < L; ++t) {
    const TowerConst& c = tcs[t];
    const uint64_t y = yf(t);
    const uint32_t ytop = __builtin_amdgcn_alignbit((uint32_t)(y >> 32), (uint32_t)y, c.crt_sh);
    f = __fadd_rn(f, __fmul_rn((float)ytop, c.inv_q32));
    const uint32_t a = (uint32_t)y & M30, b = (uint32_t)(y >> 30);
    sc[0] += (uint64_t)a * c.crt30[0];
#pragma unroll
    for (int j = 1; j < NC; ++j) sc[j] += (uint64_t)a * c.crt30[j] + (uint64_t)b * c.crt30[j - 1];
  }
  const uint32_t kk = (uint32_t)__fadd_rn(f, 0.5f);  // <= L
  const uint32_t* nq = tcs[0].nq30;
  sc[0] += (uint64_t)kk * nq[0];
#pragma unroll
  for (int j = 1; j < NC; ++j) sc[j] += (uint64_t)kk * nq[j] + (sc[j - 1] >> 30);
  uint64_t xlo = (sc[0] & M30) | ((sc[1] & M30) << 30) | (sc[2] << 60);
  uint64_t xhi = ((sc[2] & M30) >> 4) | ((sc[3] & M30) << 26) | (sc[4] << 56);
  // bits 127 .. 30 NC - 1 must be X's sign
  const bool neg = (int64_t)xhi < 0;
  const uint32_t ext = neg ? M30 : 0u;
  bool bad = (((uint32_t)sc[4] & M30) >> 7) != (ext >> 7);
#pragma unroll
  for (int j = 5; j < NC; ++j) bad |= ((uint32_t)sc[j] & M30) != ext;
  wide |= bad;
  // sign-magnitude -> double (the oracle's or_i128_to_double)
  if (neg) {
    xlo = ~xlo + 1;
    xhi = ~xhi + (xlo == 0 ? 1 : 0);
  }
  if constexpr (EDGE) {  // |X'| >= (Q - 1) / 2 - floor(Q 2^-16): k may be off by one
    const uint64_t elo = tcs[0].crt_edge[0], ehi = tcs[0].crt_edge[1];
    wide |= xhi > ehi || (xhi == ehi && xlo >= elo);
  }
  double v =__dadd_rn(__dmul_rn((double)xhi, 18446744073709551616.0), (double)xlo);
  if (neg) v = -v;
  return __dmul_rn(v, inv_scale);
}

// Bits [pos, pos + 64) of a little-endian 30-bit-limb integer of NL limbs.
__device__ __forceinline__ uint64_t mw30_bits64(const uint64_t* a, uint32_t NL, uint32_t pos) {
  uint64_t r = 0;
#pragma unroll 1
  for (uint32_t l = pos / 30; l < NL && 30 * l < pos + 64; ++l) {
    const int sh = (int)(30 * l) - (int)pos;
    r |= sh >= 0 ? (a[l] << sh) : (a[l] >> -sh);
  }
  return r;
}

// a += m * b (mod 2^(30 NL)), a normalised to 30-bit limbs
__device__ __forceinline__ void mw30_addmul(uint64_t* a, const uint32_t* b, uint64_t m, uint32_t NL) {
  constexpr uint64_t M30 = (1u << 30) - 1;
  uint64_t carry = 0;
#pragma unroll 1
  for (uint32_t j = 0; j < NL; ++j) {
    const uint64_t v = a[j] + m * b[j] + carry;
    a[j] = v & M30;
    carry = v >> 30;
  }
}

// compare two NL-limb magnitudes: -1, 0, 1
__device__ __forceinline__ int mw30_cmp(const uint64_t* a, const uint32_t* b, uint32_t NL) {
#pragma unroll 1
  for (int j = (int)NL - 1; j >= 0; --j)
    if (a[j] != b[j]) return a[j] < b[j] ? -1 : 1;
  return 0;
}

__device__ __forceinline__ void mw30_negate(uint64_t* a, uint32_t NL) {
  constexpr uint64_t M30 = (1u << 30) - 1;
  uint64_t carry = 1;
#pragma unroll 1
  for (uint32_t j = 0; j < NL; ++j) {
    const uint64_t v = ((~a[j]) & M30) + carry;
    a[j] = v & M30;
    carry = v >> 30;
  }
}

// The exact centred CRT over any tower set (round 6; PALISADE's CRTInterpolate to a BigInteger and
// centring mod Q before Decode, ckks.cpp:189): X in [-(Q - 1) / 2, (Q - 1) / 2]
// from V = sum_t y_t (Q/q_t) (< L Q) in NL 30-bit limbs (DeviceTables::crt_mw), k = round(sum_t
// y_t / q_t) in binary64, X' = V - k Q in two's complement, then at most two corrections by Q
// against (Q - 1) / 2 (exact comparisons), so k's estimate only has to be within 1.  |X| becomes
// NW 64-bit words w and (double) by Horner from the top, d = d 2^64 + (double)w_i, the oracle's
// or_mw_to_double; leading zero words leave d unchanged, so below 2^127 this is crt_value's
// two-word conversion bit for bit.  A slow path: limbs live in scratch (private memory).
template <class YF>
__device__ __forceinline__ double crt_exact_value(YF yf, uint32_t L, const TowerConst* __restrict__ tcs,
                                                  const uint32_t* __restrict__ mw, double inv_scale) {
  constexpr uint64_t M30 = (1u << 30) - 1;
  const uint32_t NL = mw[0], NW = mw[1];
  const uint32_t* qh = mw + 4;
  const uint32_t* nQ = qh + (size_t)L * NL;
  const uint32_t* half = nQ + NL;
  uint64_t acc[kCrtMwMaxLimbs];
#pragma unroll 1
  for (uint32_t j = 0; j < NL; ++j) acc[j] = 0;
  double f = 0.0;
#pragma unroll 1
  for (uint32_t t = 0; t < L; ++t) {
    const uint64_t y = yf(t);
    f = __dadd_rn(f, __dmul_rn((double)y, tcs[t].inv_q));
    const uint64_t a = y & M30, b = y >> 30;
    const uint32_t* h = qh + (size_t)t * NL;
    uint64_t carry = 0;
#pragma unroll 1
    for (uint32_t j = 0; j < NL; ++j) {
      const uint64_t v = acc[j] + a * h[j] + (j ? b * h[j - 1] : 0) + carry;
      acc[j] = v & M30;
      carry = v >> 30;
    }
  }
  mw30_addmul(acc, nQ, (uint64_t)__dadd_rn(f, 0.5), NL);  // X' = V - k Q
#pragma unroll 1
  for (int it = 0; it < 2; ++it) {
    const bool neg = (acc[NL - 1] >> 29) & 1;
    if (!neg) {
      if (mw30_cmp(acc, half, NL) <= 0) break;
      mw30_addmul(acc, nQ, 1, NL);  // X' - Q
    } else {
      mw30_negate(acc, NL);
      const bool over = mw30_cmp(acc, half, NL) > 0;
      mw30_negate(acc, NL);
      if (!over) break;
      // X' + Q = X' - (2^(30 NL) - Q) mod 2^(30 NL)
      mw30_negate(acc, NL);
      mw30_addmul(acc, nQ, 1, NL);
      mw30_negate(acc, NL);
    }
  }
  const bool neg = (acc[NL - 1] >> 29) & 1;
  if (neg) mw30_negate(acc, NL);
  double d = (double)mw30_bits64(acc, NL, 64 * (NW - 1));
#pragma unroll 1
  for (int w = (int)NW - 2; w >= 0; --w)
    d = __dadd_rn(__dmul_rn(d, 18446744073709551616.0), (double)mw30_bits64(acc, NL, 64 * (uint32_t)w));
  if (neg) d = -d;
  return __dmul_rn(d, inv_scale);
}

// -------------------------------------------------------------- decrypt ----
// Centred CRT: y_t = b_t (Q/q_t)^-1 mod q_t; X = sum y_t (Q/q_t) - k Q with k = round(sum y_t / q_t)
// (crt_value: NC exact columns, *wide set when X is outside the 128-bit range); then (double)X *
// (1/scale) (PALISADE Decode: ConvertToDouble * scalingFactorPre * 2^-p).  Written at bitrev(i) for
// FFTSpecial.  EXACT: crt_exact_kernel's arithmetic (crt_exact_value, every |X| <= (Q - 1) / 2).
template <int NC, bool EXACT = false, bool EDGE = false>
__global__ __launch_bounds__(256) void crt_decode_kernel(const uint64_t* __restrict__ dbuf,
                                                         uint64_t K, uint32_t logN, uint32_t logS,
                                                         uint32_t L,
                                                         const TowerConst* __restrict__ tcs,
                                                         const uint32_t* __restrict__ mw,
                                                         double inv_scale,
                                                         double2* __restrict__ fbuf,
                                                         GenFlag wide_flag) {
  const uint32_t N = 1u << logN, S = 1u << logS;
  // S >= 256: a block owns the 256 slots i = hi.2^(logS-4) | mid.16 | lo (hi, lo < 16) of one
  // middle value, so the tower reads (16 consecutive i) and, after a transpose through LDS,
  // the bit-reversed stores (16 consecutive outputs, 256 B) are both contiguous.
  const bool tiled = logS >= 8;
  uint64_t k;
  uint32_t i, mid = 0;
  if (tiled) {
    k = blockIdx.x >> (logS - 8);
    mid = blockIdx.x & ((1u << (logS - 8)) - 1);
    i = ((threadIdx.x >> 4) << (logS - 4)) | (mid << 4) | (threadIdx.x & 15);
  } else {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    k = gid >> logS;
    i = (uint32_t)(gid & (S - 1));
  }
  if (k >= K) return;  // block-uniform when tiled (the grid is exact)
  const uint32_t gapLog = logN - 1 - logS;
  const uint64_t* __restrict__ d = dbuf + k * ((uint64_t)L << logN);
  double res[2];
  bool wide = false;
#pragma unroll
  for (int part = 0; part < 2; ++part) {
    const uint32_t j = (part ? (N >> 1) : 0) + (i << gapLog);
    const auto yf = [&](uint32_t t) {
      const TowerConst& c = tcs[t];
      return shoup_mul(d[((uint64_t)t << logN) + j], c.qhat_inv, c.qhat_inv_shoup, c.q);
    };
    if constexpr (EXACT)
      res[part] = crt_exact_value(yf, L, tcs, mw, inv_scale);
    else
      res[part] = crt_value<NC, EDGE>(yf, L, tcs, inv_scale, wide);
  }
  if (wide) gen_flag_set(wide_flag, 2);
  if (!tiled) {
    fbuf[k * S + bitrev_dev(i, logS)] = make_double2(res[0], res[1]);
    return;
  }
  // bitrev(i) = bitrev4(lo).2^(logS-4) | bitrev(mid).16 | bitrev4(hi): slot (lo, hi) goes to
  // tile row bitrev4(lo), column bitrev4(hi); rows padded to 17 entries (conflict-free).
  __shared__ double2 tile[16][17];
  tile[bitrev_dev(threadIdx.x & 15, 4)][bitrev_dev(threadIdx.x >> 4, 4)] = make_double2(res[0], res[1]);
  __syncthreads();
  const uint32_t a = threadIdx.x >> 4, b = threadIdx.x & 15;
  fbuf[k * S + ((a << (logS - 4)) | (bitrev_dev(mid, logS - 8) << 4) | b)] = tile[a][b];
}

// Decrypt's last INTT pass fused with the exact CRT decode (ntt_inv_cols + crt_decode_kernel
// without the round trip of the [K][L][N] residues through HBM).  A workgroup owns 64
// columns (coefficients j = c + BLK r, r < R) of one ciphertext for every tower: wave w
// runs the top LOGR stages of towers t = w, w + 4, ... and leaves y_t = b_t (N^-1 (Q/q_t)^-1)
// mod q_t in LDS; then each (real, imaginary) coefficient pair (r, r + R/2) is
// CRT-reconstructed exactly as crt_decode_kernel does (same operation order) and stored
// at bitrev(slot).  Needs L R 512 B of LDS <= kCrtFuseLds and gap = N / 2S <= 64.
// LDS rows: the CRT loop reads ys[t][r][u] with r fastest (8 consecutive lanes = 8 rows, 4
// consecutive u per 32-lane ds_read_b64 group); rows of 64 u64 would put those 8 rows on one bank.
// Round 5: column u is stored at u ^ 4 (r mod 8) -- 32 distinct banks per group in L R 512 B (32 KiB
// at 2^15 / L4, 5 workgroups per CU; the round-4 rows padded to 68 u64 ran the same, 0.960 vs 0.959
// us per decrypted ciphertext, profiles/r05d).
constexpr size_t kCrtFuseLds = 48 << 10;
template <int LOGR, int NC, bool EDGE = false>
__global__ __launch_bounds__(256) void ntt_inv_cols_crt(const uint64_t* __restrict__ dbuf, uint32_t L,
                                                        uint32_t logN, uint32_t logS,
                                                        const uint64_t* __restrict__ tw,
                                                        const uint64_t* __restrict__ twp,
                                                        const TowerConst* __restrict__ tcs, double inv_scale,
                                                        double2* __restrict__ fbuf,
                                                        GenFlag wide_flag) {
  constexpr int R = 1 << LOGR, CW = 64, CWP = 64;
  extern __shared__ uint64_t ys_flat[];  // [L][R][CWP]
  uint64_t(*ys)[R][CWP] = reinterpret_cast<uint64_t(*)[R][CWP]>(ys_flat);
  const auto ucol = [](uint32_t r, uint32_t u) { return u ^ ((r & 7u) << 2); };
  const uint32_t N = 1u << logN, BLK = N >> LOGR, S = 1u << logS;
  const uint32_t cpb = BLK / CW;
  const uint64_t k = blockIdx.x / cpb;
  const uint32_t c0 = (blockIdx.x % cpb) * CW;
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll 1
  for (uint32_t t = wv; t < L; t += 4) {
    const TowerConst& c = tcs[t];
    const uint64_t q = c.q;
    const uint64_t* __restrict__ w = tw + ((uint64_t)t << logN);
    const uint64_t* __restrict__ wp = twp + ((uint64_t)t << logN);
    const uint64_t* __restrict__ a = dbuf + ((k * L + t) << logN) + c0 + lane;
    uint64_t x[R];
#pragma unroll
    for (int r = 0; r < R; ++r) x[r] = a[(uint64_t)r * BLK];
#pragma unroll
    for (int v = 0; v < LOGR - 1; ++v) {
      const int tr = 1 << v, h = R >> (v + 1);
#pragma unroll
      for (int i = 0; i < h; ++i) {
        const uint64_t W = w[h + i], Wp = wp[h + i];
#pragma unroll
        for (int jj = 0; jj < tr; ++jj) {
          if (gs_in8<true>(v, jj))
            gs_bfly_b<true>(x[2 * i * tr + jj], x[2 * i * tr + jj + tr], W, Wp, q, c.n8q);
          else
            gs_bfly_b<false>(x[2 * i * tr + jj], x[2 * i * tr + jj + tr], W, Wp, q, c.n8q);
        }
      }
    }
    // the last stage (one twiddle, w[1]) fused with the scale N^-1 (Q/q_t)^-1 (round 5): X = (x + y) c,
    // Y = (x + B - y) (w[1] c) -- two products per pair instead of the butterfly's one and the scale's two
    constexpr int TR = R / 2;
#pragma unroll
    for (int jj = 0; jj < TR; ++jj) {
      const uint64_t xv = x[jj], yv = x[jj + TR];
      const uint64_t B = gs_in8<true>(LOGR - 1, jj) ? (q << 3) : (q << 2);  // the butterfly's input bound
      ys[t][jj][ucol(jj, lane)] = canon4(shoup_lazy(xv + yv, c.ninv_qhat, c.ninv_qhat_shoup, q), q);
      ys[t][jj + TR][ucol(jj + TR, lane)] =
          canon4(shoup_lazy(xv + B - yv, c.ninv_qhat_w1, c.ninv_qhat_w1_shoup, q), q);
    }
  }
  __syncthreads();
  const uint32_t gapLog = logN - 1 - logS, gap = 1u << gapLog;
  bool wide = false;
  // pair p -> half-row r (< R/2) fastest, so 8 consecutive threads store 8 consecutive
  // bit-reversed slots (one 128-byte segment)
#pragma unroll 1
  for (uint32_t p = threadIdx.x; p < (uint32_t)(R / 2) * CW; p += 256) {
    const uint32_t r = p % (R / 2), u = p / (R / 2);
    const uint32_t col = c0 + u;
    if (col & (gap - 1)) continue;  // coefficient not on a slot
    double res[2];
#pragma unroll
    for (int part = 0; part < 2; ++part) {
      const uint32_t rr = r + part * (R / 2);
      res[part] =
          crt_value<NC, EDGE>([&](uint32_t t) { return ys[t][rr][ucol(rr, u)]; }, L, tcs, inv_scale, wide);
    }
    const uint32_t i = (col + BLK * r) >> gapLog;
    fbuf[k * S + bitrev_dev(i, logS)] = make_double2(res[0], res[1]);
  }
  if (wide) gen_flag_set(wide_flag, 2);
}

// ------------------------------------------------- decode noise flooding ----
// PALISADE 1.11 CKKSPackedEncoding::Decode, on the coefficient
// pairs v_i = (c[i gap], c[N/2 + i gap]) / scale that crt_decode_kernel wrote at
// bitrev(i).  m(X^-1) in this packing is conj_0 = (re_0, -im_0),
// conj_i = (-im_{S-i}, -re_{S-i}); the anti-symmetric part u = v - conj has S
// independent components (i = 0: 2 im_0; 0 < i < S/2: both; i = S/2: one), whose
// sample stddev / 2 estimates the decryption error sigma.  In 2^p units (p = scale
// bits, PALISADE's plaintext modulus): fail if log2 sigma > p - 5; sigma >= sqrt(N)/8;
// stddev = sqrt(M+1) sigma; each output becomes (v + conj)/2 + 2^-p N(0, stddev);
// logError = round(log2(stddev sqrt(2 S))).  One block per ciphertext.
__device__ __forceinline__ double block_sum_1024(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red[wave] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x < 64) {
    s = threadIdx.x < (blockDim.x >> 6) ? red[threadIdx.x] : 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if (threadIdx.x == 0) red[16] = s;
  }
  __syncthreads();
  s = red[16];
  __syncthreads();
  return s;
}

// (box_muller: dev_common.h)
// (re, im) normals of FFT-input position P: ChaCha20 block P >> 3 (nonce (3 << 56) | g),
// stream words 2 (P mod 8) and 2 (P mod 8) + 1 (one u64 of chacha20_block's output).
__device__ __forceinline__ void flood_pair(uint64_t w, double& z0, double& z1) {
  box_muller((uint32_t)w, (uint32_t)(w >> 32), z0, z1);
}

__global__ __launch_bounds__(1024) void decode_flood_kernel(double2* __restrict__ fbuf, uint32_t logS,
                                                            uint32_t logN, double two_p,
                                                            double p_bits, double m_factor,
                                                            Key8 key, uint64_t g0,
                                                            uint32_t* __restrict__ flags, GenFlag fail) {
  __shared__ double red[17];
  const uint32_t S = 1u << logS, half = S >> 1;
  double2* __restrict__ f = fbuf + (uint64_t)blockIdx.x * S;
  // u components of pair index i in [0, S/2]
  auto comps = [&](uint32_t i, double& a, double& b) -> int {
    const double2 x = f[bitrev_dev(i, logS)];
    if (i == 0) {
      a = 2.0 * x.y;
      return 1;
    }
    if (i == half) {
      a = x.x + x.y;
      return 1;
    }
    const double2 y = f[bitrev_dev(S - i, logS)];
    a = x.x + y.y;
    b = x.y + y.x;
    return 2;
  };
  double sigma;
  if (S == 1) {
    sigma = fabs(f[0].y);  // PALISADE StdDev: vec[0].imag() for one slot
  } else {
    double s1 = 0.0;
    for (uint32_t i = threadIdx.x; i <= half; i += blockDim.x) {
      double a = 0.0, b = 0.0;
      const int c = comps(i, a, b);
      s1 += a + (c == 2 ? b : 0.0);
    }
    const double mean = block_sum_1024(s1, red) / (double)S;
    double s2 = 0.0;
    for (uint32_t i = threadIdx.x; i <= half; i += blockDim.x) {
      double a = 0.0, b = 0.0;
      const int c = comps(i, a, b);
      s2 += (a - mean) * (a - mean) + (c == 2 ? (b - mean) * (b - mean) : 0.0);
    }
    const double var = block_sum_1024(s2, red) / (double)(S - 1);
    sigma = 0.5 * sqrt(var);
  }
  double sigma_p = sigma * two_p;  // PALISADE works at scale 2^p
  const double logstd = log2(sigma_p);
  if (!(logstd <= p_bits - 5.0)) {
    if (threadIdx.x == 0) gen_flag_set(fail, 3);  // decode precision failure
  }
  const double floor_sd = 0.125 * sqrt((double)(1u << logN));
  if (sigma_p < floor_sd) sigma_p = floor_sd;
  const double stddev_p = sqrt(m_factor + 1.0) * sigma_p;
  if (threadIdx.x == 0) {
    const double le = rint(log2(stddev_p * sqrt(2.0 * (double)S)));
    atomicMax((int*)&flags[2], (int)le);
  }
  const double nsd = stddev_p / two_p;  // noise stddev in output units
  const uint64_t nonce = (3ull << 56) | (g0 + blockIdx.x);
  // the normals of the slot at FFT-input position P: block P >> 1, pair P & 1
  auto noise = [&](uint32_t P, double& za, double& zb) {
    uint64_t w[8];
    chacha20_block(key, P >> 3, nonce, w);
    flood_pair(w[P & 7], za, zb);
  };
  __syncthreads();  // every thread has read its pairs before any is overwritten
  for (uint32_t i = threadIdx.x; i <= half; i += blockDim.x) {
    const uint32_t pi = bitrev_dev(i, logS);
    const double2 x = f[pi];
    double z0, z1;
    noise(pi, z0, z1);
    if (i == 0) {
      f[pi] = make_double2(x.x + nsd * z0, nsd * z1);
      if (S == 1) continue;
    } else if (i == half) {
      f[pi] = make_double2(0.5 * (x.x - x.y) + nsd * z0, 0.5 * (x.y - x.x) + nsd * z1);
    } else {
      const uint32_t pj = bitrev_dev(S - i, logS);
      const double2 y = f[pj];
      double z2, z3;
      noise(pj, z2, z3);
      f[pi] = make_double2(0.5 * (x.x - y.y) + nsd * z0, 0.5 * (x.y - y.x) + nsd * z1);
      f[pj] = make_double2(0.5 * (y.x - x.y) + nsd * z2, 0.5 * (y.y - x.x) + nsd * z3);
    }
  }
}

// Flooding at 2^11 slots and more, in two steps that stream the slots once each:
//  1. decode_stats_kernel: per ciphertext G = S/2048 workgroups sum the anti-symmetric
//     components u (decode_flood_kernel's, over pairs (i, S - i)) and their squares;
//  2. fft_fwd_blocks adds the noise while it loads its block (FloodArgs): sigma from
//     the G partial sums (one-pass variance (sum u^2 - (sum u)^2 / S) / (S - 1)), the
//     normals of position P from ChaCha20 block P >> 3 (a thread loads positions 8m ..
//     8m + 7: one block, eight Box-Muller pairs).
// The symmetrization (v + conj)/2 is left out: conj contributes only the imaginary part
// of each decoded slot (m(1/zeta) = conj m(zeta) for real coefficients) and decrypt
// keeps real parts, so the output is the same up to rounding (oracle tolerance 1e-14).
// Slot i sits at FFT-input position P = bitrev(i); its conjugate partner S - i sits at
// P ^ (2^h - 1), h = the index of P's leading bit (complementing i's bits above its
// lowest set bit complements P's bits below its highest): the octave [2^h, 2^(h+1))
// mirrored.  Pair m (0 <= m < S/2 - 1) is P = 2^h + o with m + 1 = 2^(h-1) + o, partner
// 2^(h+1) - 1 - o: consecutive m read two contiguous runs (one backwards).  Positions 0
// (slot 0) and 1 (slot S/2) are their own partners.
constexpr uint32_t kFloodPairsPerWg = 1024;
__global__ __launch_bounds__(256) void decode_stats_kernel(const double2* __restrict__ fbuf, uint32_t logS,
                                                           uint32_t G, double2* __restrict__ part,
                                                           uint32_t* __restrict__ reset_flags) {
  __shared__ double red[2][4];
  // the call's precision / logError flags, reset here (the FFT pass that sets them runs after this
  // kernel on the same stream) instead of by a separate fill launch
  if (reset_flags && blockIdx.x == 0 && threadIdx.x < 2) reset_flags[1 + threadIdx.x] = 0;
  const uint32_t S = 1u << logS, half = S >> 1;
  const uint64_t k = blockIdx.x / G;
  const uint32_t wg = blockIdx.x % G;
  const double2* __restrict__ f = fbuf + k * S;
  double s1 = 0.0, s2 = 0.0;
  const uint32_t m1 = min(half - 1, (wg + 1) * kFloodPairsPerWg);
  for (uint32_t m = wg * kFloodPairsPerWg + threadIdx.x; m < m1; m += 256) {
    const uint32_t hb = 31 - __clz(m + 1);  // h - 1
    const uint32_t o = m + 1 - (1u << hb);
    const double2 x = f[(2u << hb) + o], y = f[(4u << hb) - 1 - o];
    const double a = x.x + y.y, b = x.y + y.x;
    s1 += a + b;
    s2 += a * a + b * b;
  }
  if (wg == 0 && threadIdx.x == 0) {
    const double2 x0 = f[0], xh = f[1];  // slot 0: 2 im; slot S/2: re + im
    const double a = 2.0 * x0.y, c = xh.x + xh.y;
    s1 += a + c;
    s2 += a * a + c * c;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s1 += __shfl_down(s1, o, 64);
    s2 += __shfl_down(s2, o, 64);
  }
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[0][wave] = s1;
    red[1][wave] = s2;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    part[blockIdx.x] = make_double2((red[0][0] + red[0][1]) + (red[0][2] + red[0][3]),
                                    (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]));
}

struct FloodArgs {
  const double2* part;  // [K][G] (sum u, sum u^2) of decode_stats_kernel
  uint32_t G, logN;
  double two_p, p_bits, m_factor;
  Key8 key;
  uint64_t g0;
  uint32_t* flags;  // [2] = max logError
  GenFlag fail;     // word 3: precision failure
};

// Ciphertext k's flooding scale from decode_stats_kernel's partial sums: the noise's standard
// deviation in slot units (the first block of each ciphertext records the precision failure and
// logError).
__device__ __forceinline__ double flood_nsd_sums(const FloodArgs& fa, double s1, double s2, uint32_t b, uint32_t S) {
  const double var = (s2 - s1 * (s1 / (double)S)) / (double)(S - 1);
  double sigma_p = 0.5 * sqrt(var > 0.0 ? var : 0.0) * fa.two_p;
  const bool fail = !(log2(sigma_p) <= fa.p_bits - 5.0);
  const double floor_sd = 0.125 * sqrt((double)(1u << fa.logN));
  if (sigma_p < floor_sd) sigma_p = floor_sd;
  const double stddev_p = sqrt(fa.m_factor + 1.0) * sigma_p;
  if (b == 0 && threadIdx.x == 0) {
    if (fail) gen_flag_set(fa.fail, 3);
    atomicMax((int*)&fa.flags[2], (int)rint(log2(stddev_p * sqrt(2.0 * (double)S))));
  }
  return stddev_p / fa.two_p;
}
__device__ __forceinline__ double flood_nsd(const FloodArgs& fa, uint64_t k, uint32_t b, uint32_t S) {
  double s1 = 0.0, s2 = 0.0;
  for (uint32_t g = 0; g < fa.G; ++g) {
    const double2 v = fa.part[k * fa.G + g];
    s1 += v.x;
    s2 += v.y;
  }
  return flood_nsd_sums(fa, s1, s2, b, S);
}

// FFTSpecial first pass (decode): input already bit-reversed by the CRT's scatter; DIT
// stages len = 2..blk with twiddle ffwd[len/2 + (x mod len)] in LDS blocks; the top LOGR
// stages follow on register columns (fft_fwd_cols).  A single pass writes the real parts
// of the first `n` slots straight into the caller's output vector; FLOOD adds the decode
// noise there, in the output domain (as fft_fwd_cols).
// Decoded slot gi into the call's n output values.  Real packing: its real part at out[gi].  Complex packing
// (CX): (re, im) at out[2 gi], out[2 gi + 1] as one aligned 16-byte word, under the same
// n-tail rule (the pair whose first value is out[n - 1] stores only that).
template <bool CX>
__device__ __forceinline__ void dec_slot(double* __restrict__ out, uint64_t n, uint64_t gi, double2 v) {
  if constexpr (CX) {
    if (2 * gi + 1 < n)
      reinterpret_cast<double2*>(out)[gi] = v;
    else if (2 * gi < n)
      out[2 * gi] = v.x;
  } else {
    if (gi < n) out[gi] = v.x;
  }
}

// (fft_fwd_blocks and fft_fwd_whole are bodies shared by a real and a both-parts (_cx) entry point, so the
// real forms keep their names and their code; FLOOD and STATS have no complex form)
template <bool FLOOD, bool CX>
__device__ __forceinline__ void fft_fwd_blocks_body(double2* __restrict__ buf, uint32_t logS,
                                                    uint32_t blkLog, const double2* __restrict__ tw,
                                                    double* __restrict__ out, uint64_t n,
                                                    int final_pass, FloodArgs fa) {
  static_assert(!(FLOOD && CX), "flooding estimates sigma from the imaginary parts");
  extern __shared__ __attribute__((aligned(16))) double2 smc[];
  const uint32_t S = 1u << logS, blk = 1u << blkLog;
  const uint32_t sh = logS - blkLog;
  const uint64_t k = blockIdx.x >> sh;
  const uint32_t b = blockIdx.x & ((1u << sh) - 1);
  const uint64_t off = k * S + ((uint64_t)b << blkLog);
  for (uint32_t i = threadIdx.x; i < blk; i += 256) smc[i] = buf[off + i];
  __syncthreads();
  for (uint32_t len = 2; len <= blk; len <<= 1) {
    const uint32_t lenh = len >> 1;
    for (uint32_t p = threadIdx.x; p < blk / 2; p += 256) {
      const uint32_t j = p & (lenh - 1);
      const uint32_t i0 = (p - j) * 2 + j;
      const double2 W = tw[lenh + j];
      const double2 u = smc[i0];
      const double2 v = cmul(smc[i0 + lenh], W);
      smc[i0] = cadd(u, v);
      smc[i0 + lenh] = csub(u, v);
    }
    __syncthreads();
  }
  if (final_pass) {  // (one block per ciphertext: b == 0, blk == S)
    double nso = 0.0;
    uint64_t nonce = 0;
    if (FLOOD) {
      nso = flood_nsd(fa, k, b, S) * sqrt((double)S);
      nonce = (3ull << 56) | (fa.g0 + k);
    }
    for (uint32_t i = threadIdx.x; i < blk; i += 256) {
      const uint64_t gi = off + i;
      if constexpr (CX) {
        dec_slot<true>(out, n, gi, smc[i]);
        continue;
      }
      double v = smc[i].x;
      if (FLOOD) {  // fft_fwd_cols's output-domain stream: normal (i div S/16) of block (i mod S/16)
        const uint32_t S16 = S >> 4, nidx = i / S16;
        uint64_t w[8];
        chacha20_block(fa.key, i & (S16 - 1), nonce, w);
        double z0, z1;
        flood_pair(w[nidx >> 1], z0, z1);
        v = __dadd_rn(v, __dmul_rn(nso, (nidx & 1) ? z1 : z0));
      }
      if (gi < n) out[gi] = v;
    }
  } else {
    for (uint32_t i = threadIdx.x; i < blk; i += 256) buf[off + i] = smc[i];
  }
}
template <bool FLOOD>
__global__ __launch_bounds__(256) void fft_fwd_blocks(double2* __restrict__ buf, uint32_t logS,
                                                      uint32_t blkLog, const double2* __restrict__ tw,
                                                      double* __restrict__ out, uint64_t n,
                                                      int final_pass, FloodArgs fa) {
  fft_fwd_blocks_body<FLOOD, false>(buf, logS, blkLog, tw, out, n, final_pass, fa);
}
__global__ __launch_bounds__(256) void fft_fwd_blocks_cx(double2* __restrict__ buf, uint32_t logS,
                                                         uint32_t blkLog, const double2* __restrict__ tw,
                                                         double* __restrict__ out, uint64_t n,
                                                         int final_pass, FloodArgs fa) {
  fft_fwd_blocks_body<false, true>(buf, logS, blkLog, tw, out, n, final_pass, fa);
}

// FFTSpecial's first pass (decode, not the final pass): block b of ciphertext k, DIT half-sizes
// 1 .. 2^(BL-1).  (Until round 4 the flooding noise was added here, on load; it now lands on the
// output in fft_fwd_cols.)
template <int BL, int K1, int K2, int K3, int K4, bool SWZ = true>
__global__ __launch_bounds__(1 << (BL - 3)) void fft_fwd_blocks_ct(double2* __restrict__ buf, uint32_t logS,
                                                                  const double2* __restrict__ tw) {
  static_assert(K1 + K2 + K3 + K4 == BL, "chunk plan");
  __shared__ __attribute__((aligned(16))) double2 sm[1 << BL];
  const uint32_t S = 1u << logS, sh = logS - BL;
  const uint64_t k = blockIdx.x >> sh;
  const uint32_t b = blockIdx.x & ((1u << sh) - 1);
  double2* __restrict__ g = buf + k * S + ((uint64_t)b << BL);
  const auto lds_ld = [&](uint32_t j) { return sm[fft_swz<SWZ>(j)]; };
  const auto lds_st = [&](uint32_t j, double2 v) { sm[fft_swz<SWZ>(j)] = v; };
  fft_chunk<BL, K1, 0, true>(tw, [&](uint32_t j) { return g[j]; }, lds_st);
  __syncthreads();
  fft_chunk<BL, K2, K1, true>(tw, lds_ld, lds_st);
  __syncthreads();
  fft_chunk<BL, K3, K1 + K2, true>(tw, lds_ld, lds_st);
  __syncthreads();
  fft_chunk<BL, K4, K1 + K2 + K3, true>(tw, lds_ld, [&](uint32_t j, double2 v) { g[j] = v; });
}

// FFTSpecial's last pass (decode): the top LOGR stages on register columns; writes the real parts
// of the first `n` slots straight into the caller's output vector.  FLOOD (round 5): PALISADE's
// decode noise in the output domain -- N(0, sd sqrt(S)) added to each decoded real part, the same
// distribution as N(0, sd) on every FFT input (FFTSpecial's F F^H = S I; oracle or_decrypt_flood):
// slot i takes normal (i div S/16) of ChaCha20 block (i mod S/16), so a thread's 2^LOGR rows share
// 2^max(0, LOGR-4) blocks.
template <int LOGR, bool FLOOD = false>
__global__ __launch_bounds__(256) void fft_fwd_cols(const double2* __restrict__ buf, uint32_t logS,
                                                    const double2* __restrict__ tw,
                                                    double* __restrict__ out, uint64_t n, FloodArgs fa) {
  constexpr int R = 1 << LOGR;
  const uint32_t S = 1u << logS;
  const uint32_t BLK = S >> LOGR;
  const uint32_t bpp = BLK / 256;
  const uint64_t k = blockIdx.x / bpp;
  const uint32_t col = (blockIdx.x % bpp) * 256 + threadIdx.x;
  double2 v[R];
#pragma unroll
  for (int r = 0; r < R; ++r) v[r] = buf[k * S + col + (uint64_t)r * BLK];
#pragma unroll
  for (int s = 0; s < LOGR; ++s) {
    const uint32_t lenh = BLK << s;
    const int tr = 1 << s;
#pragma unroll
    for (int r0 = 0; r0 < R; ++r0) {
      if ((r0 >> s) & 1) continue;
      const int r1 = r0 + tr;
      const uint32_t j = col + (uint32_t)(r0 & ((2 << s) - 1)) * BLK;  // (col + r0 BLK) mod len
      const double2 W = tw[lenh + j];
      const double2 u = v[r0];
      const double2 w = cmul(v[r1], W);
      v[r0] = cadd(u, w);
      v[r1] = csub(u, w);
    }
  }
  if (FLOOD) {
    const double nso = flood_nsd(fa, k, blockIdx.x % bpp, S) * sqrt((double)S);
    const uint64_t nonce = (3ull << 56) | (fa.g0 + k);
    const uint32_t S16 = S >> 4;
    constexpr int LO = LOGR > 4 ? LOGR - 4 : 0;  // ChaCha blocks per thread: 2^LO
#pragma unroll
    for (int rl = 0; rl < (1 << LO); ++rl) {
      uint64_t w[8];
      chacha20_block(fa.key, (col + BLK * (uint32_t)rl) & (S16 - 1), nonce, w);
      if (LOGR >= 4) {  // the thread's rows use all 16 normals of the block
        double z[16];
#pragma unroll
        for (int m = 0; m < 8; ++m) flood_pair(w[m], z[2 * m], z[2 * m + 1]);
#pragma unroll
        for (int r = rl; r < R; r += (1 << LO)) {
          const uint32_t nidx = (col + BLK * (uint32_t)r) / S16;  // < 16
          double zr = 0.0;
#pragma unroll
          for (int m = 0; m < 16; ++m) zr = (uint32_t)m == nidx ? z[m] : zr;  // no dynamic register index
          v[r].x = __dadd_rn(v[r].x, __dmul_rn(nso, zr));
        }
      } else {  // rows 2^(4-LOGR) normals apart: one Box-Muller pair per row, half of it used
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const uint32_t nidx = (col + BLK * (uint32_t)r) / S16;
          uint64_t wr = 0;
#pragma unroll
          for (int m = 0; m < 8; ++m) wr = (uint32_t)m == (nidx >> 1) ? w[m] : wr;
          double z0, z1;
          flood_pair(wr, z0, z1);
          v[r].x = __dadd_rn(v[r].x, __dmul_rn(nso, (nidx & 1) ? z1 : z0));
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint64_t gi = k * S + col + (uint64_t)r * BLK;
    if (gi < n) out[gi] = v[r].x;
  }
}

// fft_fwd_cols<LOGR, false> for complex slot packing: both parts of every slot (dec_slot).  A kernel of its own
// (a shared body moved the flooded forms' register counts): the last stage, whose 2^LOGR outputs are all live
// here where the real form keeps only their real parts, stores each pair as it is done (as fft_fwd_whole), so
// the column holds its occupancy (register counts in DESIGN.md §2.19).
template <int LOGR>
__global__ __launch_bounds__(256) void fft_fwd_cols_cx(const double2* __restrict__ buf, uint32_t logS,
                                                       const double2* __restrict__ tw,
                                                       double* __restrict__ out, uint64_t n) {
  constexpr int R = 1 << LOGR;
  const uint32_t S = 1u << logS;
  const uint32_t BLK = S >> LOGR;
  const uint32_t bpp = BLK / 256;
  const uint64_t k = blockIdx.x / bpp;
  const uint32_t col = (blockIdx.x % bpp) * 256 + threadIdx.x;
  double2 v[R];
#pragma unroll
  for (int r = 0; r < R; ++r) v[r] = buf[k * S + col + (uint64_t)r * BLK];
#pragma unroll
  for (int s = 0; s < LOGR - 1; ++s) {
    const uint32_t lenh = BLK << s;
    const int tr = 1 << s;
#pragma unroll
    for (int r0 = 0; r0 < R; ++r0) {
      if ((r0 >> s) & 1) continue;
      const int r1 = r0 + tr;
      const uint32_t j = col + (uint32_t)(r0 & ((2 << s) - 1)) * BLK;  // (col + r0 BLK) mod len
      const double2 W = tw[lenh + j];
      const double2 u = v[r0];
      const double2 w = cmul(v[r1], W);
      v[r0] = cadd(u, w);
      v[r1] = csub(u, w);
    }
  }
#pragma unroll
  for (int r0 = 0; r0 < R / 2; ++r0) {  // the last stage: half-size S/2, rows r0 and r0 + R/2
    asm volatile("" ::: "memory");  // each pair's twiddle load and stores stay with the pair
    const int r1 = r0 + R / 2;
    const double2 W = tw[(S >> 1) + col + (uint32_t)r0 * BLK];
    const double2 w = cmul(v[r1], W);
    const uint64_t gi = k * S + col + (uint64_t)r0 * BLK;
    dec_slot<true>(out, n, gi, cadd(v[r0], w));
    dec_slot<true>(out, n, gi + (S >> 1), csub(v[r0], w));
  }
}

// decode_stats_kernel's sums inside the whole-vector decode (round 5): a[i] holds FFT-input position
// P = 1024 w + 4 (l + 64 (i >> 2)) + (i & 3); pair (P, P ^ (2^h - 1)) (h = P's leading bit, P in the
// lower half of its octave) contributes a = x.re + y.im and b = x.im + y.re, positions 0 and 1 their
// own terms.  The partners' components come through LDS (real parts, then imaginary), the sums by a
// wave shuffle and LDS reduction; every thread returns (sum, sum of squares).
__device__ __forceinline__ double2 fft_whole_flood_stats(const double2 (&a)[16], double* __restrict__ lds) {
  const uint32_t T = threadIdx.x, w = T >> 6, l = T & 63;
  double s1 = 0.0, s2 = 0.0;
#pragma unroll
  for (int part = 0; part < 2; ++part) {
#pragma unroll
    for (int i = 0; i < 16; ++i) lds[w * kFftWholeRow + fft_wt1(l, i)] = part ? a[i].y : a[i].x;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const uint32_t P = 1024 * w + 4 * (l + 64 * (i >> 2)) + (i & 3);
      if (P < 2) continue;
      const uint32_t h = 31 - __clz(P);
      if ((P >> (h - 1)) & 1) continue;  // upper half of the octave: counted by its partner
      const uint32_t Q = P ^ ((1u << h) - 1);
      const double y = lds[(Q >> 10) * kFftWholeRow + fft_wpad(Q & 1023)];
      const double v = part ? a[i].x + y : a[i].y + y;  // part 0: b = x.im + y.re; part 1: a = x.re + y.im
      s1 += v;
      s2 += v * v;
    }
    __syncthreads();
  }
  if (T == 0) {  // slot 0: 2 im; slot S/2: re + im (positions 0 and 1)
    const double a0 = 2.0 * a[0].y, c = a[1].x + a[1].y;
    s1 += a0 + c;
    s2 += a0 * a0 + c * c;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s1 += __shfl_down(s1, o, 64);
    s2 += __shfl_down(s2, o, 64);
  }
  if (l == 0) {
    lds[2 * w] = s1;
    lds[2 * w + 1] = s2;
  }
  __syncthreads();
  double t1 = 0.0, t2 = 0.0;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    t1 += lds[2 * v];
    t2 += lds[2 * v + 1];
  }
  __syncthreads();  // the LDS is the block exchanges' next
  return make_double2(t1, t2);
}

// FFTSpecial (decode) of one 2^14-slot vector per workgroup (see fft_inv_whole): buf [K][S] (bit-reversed
// by the CRT's scatter) -> the real parts of the first n slots in out.  STATS (flooded decrypts): the
// workgroup also sums decode_stats_kernel's statistics of its vector (fft_whole_flood_stats) into
// part[k]; flood_add_kernel then adds the noise to out (adding it here, beside the 16 values per thread,
// spilled under the 128-VGPR cap and ran slower than the extra pass).
template <bool STATS, bool CX>
__device__ __forceinline__ void fft_fwd_whole_body(const double2* __restrict__ buf, const double2* __restrict__ tw,
                                                   double* __restrict__ out, uint64_t n,
                                                   double2* __restrict__ part) {
  static_assert(!(STATS && CX), "flooding estimates sigma from the imaginary parts");
  constexpr uint32_t S = 1u << kFftWholeLogS, BLK = 1024;
  constexpr int R = 16;
  __shared__ double lds[16 * kFftWholeRow];
  const uint64_t k = blockIdx.x;
  const uint32_t T = threadIdx.x, w = T >> 6, l = T & 63;
  double2 a[R];
  // block w: DIT half-sizes 1 .. 2 on sets l + 64 q (elements 4 (l + 64 q) + m), loaded from HBM
  const double2* __restrict__ g = buf + k * S + (uint64_t)w * BLK;
#pragma unroll
  for (int i = 0; i < R; ++i) a[i] = g[4 * (l + 64 * (i >> 2)) + (i & 3)];
  if (STATS) {
    const double2 st = fft_whole_flood_stats(a, lds);
    if (T == 0) part[k] = st;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    double2 c[4] = {a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]};
    fft_dit_set<2, 0>(c, 0u, tw);
#pragma unroll
    for (int m = 0; m < 4; ++m) a[4 * q + m] = c[m];
  }
  double* Ls = lds + w * kFftWholeRow;
  // (the empty asm statements keep each phase's twiddle loads in that phase: hoisted to the kernel
  // entry, 33 twiddles would not fit beside the data under the 128-VGPR cap)
  fft_wave_xch(a, Ls, [&](int m) { return fft_xa1(l, m); }, [&](int m) { return fft_xa2(l, m); });
  asm volatile("" ::: "memory");
  fft_dit_set<4, 2>(a, l & 3, tw);  // half-sizes 4 .. 32
  fft_wave_xch(a, Ls, [&](int m) { return fft_xb2(l, m); }, [&](int m) { return fft_xb3(l, m); });
  asm volatile("" ::: "memory");
  fft_dit_set<4, 6>(a, l, tw);  // half-sizes 64 .. 512
  asm volatile("" ::: "memory");
  fft_whole_transpose<false>(a, lds);
  // columns: DIT half-sizes 1024 .. 4096 on column T (fft_fwd_cols<4>); the last stage (8192) computes
  // only the real parts decrypt returns and stores each pair as it is done (with every output held to the
  // end, the column pass spilled under the 128-VGPR cap)
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    asm volatile("" ::: "memory");
    const uint32_t lenh = BLK << s;
    const int tr = 1 << s;
#pragma unroll
    for (int r0 = 0; r0 < R; ++r0) {
      if ((r0 >> s) & 1) continue;
      const int r1 = r0 + tr;
      const double2 W = tw[lenh + T + (uint32_t)(r0 & ((2 << s) - 1)) * BLK];
      const double2 u = a[r0];
      const double2 v = cmul(a[r1], W);
      a[r0] = cadd(u, v);
      a[r1] = csub(u, v);
    }
  }
  // uniform base + 32-bit offsets (16 precomputed 64-bit addresses would not fit)
  // (CX: the vector's 2 S values, both parts of each pair of the last stage)
  constexpr uint32_t VS = CX ? 2 * S : S;
  double* __restrict__ ok = out + k * VS;
  const uint32_t rem = n > k * VS ? (uint32_t)std::min<uint64_t>(n - k * VS, VS) : 0u;
#pragma unroll
  for (int r0 = 0; r0 < R / 2; ++r0) {
    asm volatile("" ::: "memory");
    const int r1 = r0 + R / 2;
    const double2 W = tw[(BLK << 3) + T + (uint32_t)r0 * BLK];
    const uint32_t i0 = T + (uint32_t)r0 * BLK, i1 = T + (uint32_t)r1 * BLK;
    if constexpr (CX) {
      const double2 v = cmul(a[r1], W);
      dec_slot<true>(ok, rem, i0, cadd(a[r0], v));
      dec_slot<true>(ok, rem, i1, csub(a[r0], v));
    } else {
      const double vx = __dsub_rn(__dmul_rn(a[r1].x, W.x), __dmul_rn(a[r1].y, W.y));  // cmul(a[r1], W).x
      if (i0 < rem) ok[i0] = __dadd_rn(a[r0].x, vx);
      if (i1 < rem) ok[i1] = __dsub_rn(a[r0].x, vx);
    }
  }
}
template <bool STATS>
__global__ __launch_bounds__(1024) void fft_fwd_whole(const double2* __restrict__ buf, const double2* __restrict__ tw,
                                                      double* __restrict__ out, uint64_t n,
                                                      double2* __restrict__ part) {
  fft_fwd_whole_body<STATS, false>(buf, tw, out, n, part);
}
__global__ __launch_bounds__(1024) void fft_fwd_whole_cx(const double2* __restrict__ buf, const double2* __restrict__ tw,
                                                         double* __restrict__ out, uint64_t n,
                                                         double2* __restrict__ part) {
  fft_fwd_whole_body<false, true>(buf, tw, out, n, part);
}

// The decode noise of a flooded whole-vector decode, added to the decoded outputs (fft_fwd_cols<LOGR,
// true>'s stream: slot i takes normal i div S/16 of ChaCha20 block i mod S/16): one thread per (ciphertext,
// block), 16 outputs each; sigma from the workgroup sums of fft_fwd_whole<true> (FloodArgs::part, G = 1).
__global__ __launch_bounds__(256) void flood_add_kernel(double* __restrict__ out, uint64_t n, uint32_t logS,
                                                        uint64_t K, FloodArgs fa) {
  const uint32_t S = 1u << logS, S16 = S >> 4;
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= K * S16) return;
  const uint64_t k = t / S16;
  const uint32_t b = (uint32_t)(t % S16);
  const double nso = flood_nsd(fa, k, b == 0 ? 0u : 1u, S) * sqrt((double)S);  // b == 0 records the flags
  uint64_t wd[8];
  chacha20_block(fa.key, b, (3ull << 56) | (fa.g0 + k), wd);
  double* __restrict__ ok = out + k * S;
  const uint32_t rem = n > k * S ? (uint32_t)std::min<uint64_t>(n - k * S, S) : 0u;
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    double z0, z1;
    flood_pair(wd[m], z0, z1);
    const uint32_t i0 = b + S16 * (2 * m), i1 = i0 + S16;
    if (i0 < rem) ok[i0] = __dadd_rn(ok[i0], __dmul_rn(nso, z0));
    if (i1 < rem) ok[i1] = __dadd_rn(ok[i1], __dmul_rn(nso, z1));
  }
}

// launch_decrypt: the persistent first INTT pass (ntt_inv_blocks_dec_pp) from this many (ciphertext, decode
// tower, 2^11 block) items, the one-shot ntt_inv_blocks_dec_ct below.  Decrypt / flooded us/ct, one-shot vs
// persistent (profiles/r06f/dpk_*, ppk_*): 2^15 / 3 decode towers K = 4 9.96 / 12.53 vs 10.37 / 13.07, K = 64
// (3,072 items) 1.52 / 1.75 vs 1.55 / 1.82, K = 96 (4,608) 1.53 / 1.67 vs 1.43 / 1.55; 2^16 K = 32 (3,072)
// 3.17-3.28 / 3.59-3.70 vs 3.30 / 3.73, K = 64 (6,144) 3.00 / 3.19 vs 2.76-2.84 / 2.92
constexpr uint64_t kDecPpMinItems = 4096;

static uint32_t flood_groups(uint32_t S) {
  const uint32_t half = S / 2;
  return half >= kFloodPairsPerWg ? half / kFloodPairsPerWg : 1;
}

size_t decrypt_scratch_bytes(const Params& p, uint64_t K) {
  // dbuf [K][L][N] | fbuf [K][S] | flooding partial sums [K][G]
  return K * (uint64_t)p.L * p.N * sizeof(uint64_t) + K * (uint64_t)p.batch * sizeof(double2) +
         K * (uint64_t)flood_groups(p.batch) * sizeof(double2) + 64;
}

void launch_decrypt(const Params& p, const DeviceTables& dt, const DeviceKeys& dk,
                    const uint64_t* ct, uint64_t K, double scale, uint64_t n, double* out,
                    void* scratch, hipStream_t s, const DecodeNoise* dn, bool sum_in, uint32_t ct_L,
                    GenFlag crt_flag, bool exact, const FuseIn* fuse_in) {
  if (!K) return;
  const bool cx = p.pack != 0;  // both parts of every slot: the final writers' _cx forms
  if (cx && dn && dn->enabled)
    throw Error{SHELFI_ERR_STATE, "decrypt: decode noise flooding cannot run on complex slots"};
  if (!ct_L) ct_L = p.L;
  if (ct_L < p.L) throw Error{SHELFI_ERR_ARG, "decrypt: fewer ciphertext towers than decoded towers"};
  exact = exact || dt.crt_nc == 0;  // towers too wide for crt_value's columns: always exact
  if (exact && !dt.crt_mw) throw Error{SHELFI_ERR_STATE, "decrypt: no exact CRT table for these towers"};
  if (!exact && !crt_flag.p) throw Error{SHELFI_ERR_STATE, "decrypt: the fast CRT needs a range flag"};
  // a chain at or below 2^130, decoded whole: the kernels' EDGE variants (crt_value), 5 columns
  const bool edge = !exact && dt.crt_edge;
  if (edge && dt.crt_nc != 5) throw Error{SHELFI_ERR_STATE, "decrypt: a short chain needs 5 CRT columns"};
  const uint32_t logS = __builtin_ctz(p.batch);
  uint64_t* dbuf = reinterpret_cast<uint64_t*>(scratch);
  double2* fbuf = reinterpret_cast<double2*>(dbuf + K * (uint64_t)p.L * p.N);
  // c0 + c1*s formed in the first INTT pass (ntt_inv_blocks reading the ciphertexts); the
  // last pass fused with the CRT decode where its shape allows
  const uint32_t blkLog = ntt_block_log(p.logN);
  const int logR = (int)(p.logN - blkLog);
  const size_t fuse_lds = (size_t)p.L * 64 * sizeof(uint64_t) << (logR > 0 ? logR : 0);
  // (the fused pass has no 64-row form: logR = 6, ring 2^17 over 2^11 blocks, whose one-tower chain
  // would fit the LDS bound, takes the unfused pair)
  const bool fuse = !exact && logR > 0 && logR <= 5 && fuse_lds <= kCrtFuseLds && p.gap <= 64 &&
                    ((p.N >> logR) % 64) == 0;
  {
    const uint64_t P = K * p.L, nbBlocks = P << logR;
    if (nbBlocks > 0x7FFFFFFFull) throw Error{SHELFI_ERR_ARG, "decrypt batch too large"};
    const uint32_t xg = xcd_combos(p.L << (logR > 0 ? logR : 0));
    // the persistent pass from kDecPpMinItems (ciphertext, tower, block) items: below, its per-workgroup
    // prologue is not amortised and the one-shot pass is faster (same dbuf bits)
    const bool pp = logR > 0 && blkLog == 11 && dt.red_ok && switches().dec_pp &&
                    K * ((uint64_t)p.L << logR) >= kDecPpMinItems;
    // One choice for both inputs.  NoFuse reads the ciphertexts and the key; FuseIn (threshold fusion) reads
    // the partials instead (ct, dk unused): always SUM, and the generic kernel folds them itself (sum_in 0).
    const auto first_pass = [&](auto fz, const uint64_t* c, const uint64_t* sk, const uint64_t* sksh) {
      using FZ = decltype(fz);
      constexpr bool FUSE = std::is_same<FZ, FuseIn>::value;
      const bool sum = FUSE || sum_in;  // (SUM = FUSE below: false for NoFuse; FuseIn has only SUM = true forms)
#define DEC_PP(SUM, WL)                                                                                          \
  hipLaunchKernelGGL((ntt_inv_blocks_dec_pp<11, 2, 3, 3, 3, SUM, WL, FZ>), dim3(ncombo * pc), dim3(256), 0, s, dbuf, \
                     p.L, p.logN, dt.tw_inv_blk, dt.tc, c, sk, sksh, (uint32_t)K, pc, ct_L, fz)
#define DEC_CT(BL, K1, SUM)                                                                                      \
  hipLaunchKernelGGL((ntt_inv_blocks_dec_ct<BL, K1, 3, 3, 3, SUM, FZ>), dim3((uint32_t)nbBlocks), dim3(256), 0, s,  \
                     dbuf, p.L, p.logN, dt.tw_inv_blk, dt.tc, c, sk, sksh, xg, ct_L, fz)
      if (pp) {
        const uint32_t ncombo = p.L << logR;
        const uint32_t pc = pp_per_combo(ncombo, K, 3);
        if (!FUSE && sum_in) DEC_PP(true, false);  // summed ciphertexts: SUM, and no wave-local form
        else if (ntt_wave_local()) DEC_PP(FUSE, true);
        else DEC_PP(FUSE, false);
      } else if (logR > 0 && blkLog == 11 && dt.red_ok) {
        if (sum) DEC_CT(11, 2, true);
        else DEC_CT(11, 2, FUSE);
      } else if (logR > 0 && blkLog == 12 && dt.red_ok) {
        if (sum) DEC_CT(12, 3, true);
        else DEC_CT(12, 3, FUSE);
      } else
        hipLaunchKernelGGL(ntt_inv_blocks<FZ>, dim3((uint32_t)nbBlocks), dim3(256), sizeof(uint64_t) << blkLog, s,
                           dbuf, p.L, p.logN, blkLog, dt.ipsi_rev, dt.ipsi_rev_sh, dt.tc, logR == 0 ? 1 : 0, c, sk,
                           sksh, !FUSE && sum_in ? 1 : 0, ct_L, fz);
#undef DEC_CT
#undef DEC_PP
    };
    if (fuse_in)
      first_pass(*fuse_in, nullptr, nullptr, nullptr);
    else
      first_pass(NoFuse{}, ct, dk.sk, dk.sk_sh);
    if (logR > 0 && fuse) {
      const uint64_t nbf = K * ((p.N >> logR) / 64);
#define CRT_FUSED(LR, NCC, EDGE)                                                                              \
  hipLaunchKernelGGL((ntt_inv_cols_crt<LR, NCC, EDGE>), dim3((uint32_t)nbf), dim3(256), fuse_lds, s, dbuf, p.L, \
                     p.logN, logS, dt.ipsi_rev, dt.ipsi_rev_sh, dt.tc, 1.0 / scale, fbuf, crt_flag)
#define CRT_FUSED_NC(LR)                                  \
  if (edge) CRT_FUSED(LR, 5, true);                       \
  else if (dt.crt_nc == 5) CRT_FUSED(LR, 5, false);       \
  else if (dt.crt_nc == 6) CRT_FUSED(LR, 6, false);       \
  else CRT_FUSED(LR, 7, false);
      switch (logR) {
        case 1: CRT_FUSED_NC(1) break;
        case 2: CRT_FUSED_NC(2) break;
        case 3: CRT_FUSED_NC(3) break;
        case 4: CRT_FUSED_NC(4) break;
        case 5: CRT_FUSED_NC(5) break;
        default: throw Error{SHELFI_ERR_ARG, "unsupported ring dimension"};
      }
#undef CRT_FUSED_NC
#undef CRT_FUSED
    } else {
      launch_ntt_cols(dbuf, P, p.L, p.logN, true, dt, s);  // ntt_inv_cols (nothing when logR == 0)
    }
    SHELFI_HIP(hipGetLastError());
  }
  const uint64_t slots = K * (uint64_t)p.batch;
  if (!fuse) {
    const dim3 cg((uint32_t)((slots + 255) / 256));
#define CRT_DECODE(...)                                                                                      \
  hipLaunchKernelGGL((crt_decode_kernel<__VA_ARGS__>), cg, dim3(256), 0, s, dbuf, K, p.logN, logS, p.L, dt.tc, \
                     dt.crt_mw, 1.0 / scale, fbuf, crt_flag)
    if (exact) CRT_DECODE(5, true);
    else if (edge) CRT_DECODE(5, false, true);
    else if (dt.crt_nc == 5) CRT_DECODE(5);
    else if (dt.crt_nc == 6) CRT_DECODE(6);
    else CRT_DECODE(7);
#undef CRT_DECODE
  }
  SHELFI_HIP(hipGetLastError());
  const uint32_t fblkLog = fft_block_log(logS);
  const int flogR = (int)(logS - fblkLog);
  const size_t lds = sizeof(double2) << fblkLog;
  FloodArgs fa{};
  bool fused_flood = false;
  const bool whole = logS == kFftWholeLogS && K >= kFftWholeMinK && switches().fft_whole;  // fft_fwd_whole
  if (dn && dn->enabled) {
    for (int i = 0; i < 8; ++i) fa.key.k[i] = dn->key[i];
    fa.two_p = ldexp(1.0, (int)dn->p_bits);
    fa.p_bits = (double)dn->p_bits;
    fa.m_factor = dn->m_factor;
    fa.g0 = dn->g0;
    fa.flags = dn->flags;
    fa.fail = dn->fail;
    fa.logN = p.logN;
    fused_flood = p.batch >= 64;  // decode_flood_kernel below 2^6 slots
    if (fused_flood && whole) {  // fft_fwd_whole<true> sums its own statistics
      if (dn->reset) SHELFI_HIP(hipMemsetAsync(dn->flags + 1, 0, 8, s));
    } else if (fused_flood) {
      fa.G = flood_groups(p.batch);
      double2* part = fbuf + K * (uint64_t)p.batch;
      fa.part = part;
      hipLaunchKernelGGL(decode_stats_kernel, dim3((uint32_t)(K * fa.G)), dim3(256), 0, s, fbuf, logS, fa.G,
                         part, dn->reset ? dn->flags : (uint32_t*)nullptr);
    } else {
      if (dn->reset) SHELFI_HIP(hipMemsetAsync(dn->flags + 1, 0, 8, s));
      hipLaunchKernelGGL(decode_flood_kernel, dim3((uint32_t)K), dim3(1024), 0, s, fbuf, logS, p.logN,
                         fa.two_p, fa.p_bits, fa.m_factor, fa.key, fa.g0, fa.flags, fa.fail);
    }
    SHELFI_HIP(hipGetLastError());
  }
  if (whole) {  // one workgroup per vector, no HBM intermediate
    if (fused_flood) {
      double2* part = fbuf + K * (uint64_t)p.batch;  // [K] sums (G = 1)
      fa.part = part;
      fa.G = 1;
      hipLaunchKernelGGL(fft_fwd_whole<true>, dim3((uint32_t)K), dim3(1024), 0, s, fbuf, dt.fft_fwd, out, n, part);
      SHELFI_HIP(hipGetLastError());
      const uint64_t th = K * (p.batch >> 4);
      hipLaunchKernelGGL(flood_add_kernel, dim3((uint32_t)((th + 255) / 256)), dim3(256), 0, s, out, n, logS, K, fa);
    } else {
      hipLaunchKernelGGL(cx ? fft_fwd_whole_cx : fft_fwd_whole<false>, dim3((uint32_t)K), dim3(1024), 0, s, fbuf,
                         dt.fft_fwd, out, n, (double2*)nullptr);
    }
    SHELFI_HIP(hipGetLastError());
    return;
  }
  const bool fct = flogR > 0 && (fblkLog == 10 || fblkLog == 11) && switches().fft_ct;
  const dim3 fg((uint32_t)(K << flogR));
  // the flooding noise lands on the pass that writes the output (fft_fwd_cols, or the single pass)
  if (fct && fblkLog == 10)
    hipLaunchKernelGGL((fft_fwd_blocks_ct<10, 3, 3, 2, 2>), fg, dim3(128), 0, s, fbuf, logS, dt.fft_fwd);
  else if (fct)
    hipLaunchKernelGGL((fft_fwd_blocks_ct<11, 3, 3, 3, 2>), fg, dim3(256), 0, s, fbuf, logS, dt.fft_fwd);
  else if (fused_flood && flogR == 0)
    hipLaunchKernelGGL(fft_fwd_blocks<true>, fg, dim3(256), lds, s, fbuf, logS, fblkLog, dt.fft_fwd, out, n, 1, fa);
  else
    hipLaunchKernelGGL(cx ? fft_fwd_blocks_cx : fft_fwd_blocks<false>, fg, dim3(256), lds, s, fbuf, logS,
                       fblkLog, dt.fft_fwd, out, n, flogR == 0 ? 1 : 0, fa);
  SHELFI_HIP(hipGetLastError());
  if (flogR > 0) {
    const uint64_t nb = K * ((p.batch >> flogR) / 256);
#define COLS_FWD1(LR, FL) \
  hipLaunchKernelGGL((fft_fwd_cols<LR, FL>), dim3((uint32_t)nb), dim3(256), 0, s, fbuf, logS, dt.fft_fwd, out, n, fa)
#define COLS_FWD(LR)                                                                                                   \
  if (cx)                                                                                                              \
    hipLaunchKernelGGL(fft_fwd_cols_cx<LR>, dim3((uint32_t)nb), dim3(256), 0, s, fbuf, logS, dt.fft_fwd, out, n);     \
  else if (fused_flood) COLS_FWD1(LR, true);                                                                           \
  else COLS_FWD1(LR, false);
    switch (flogR) {
      case 1: COLS_FWD(1) break;
      case 2: COLS_FWD(2) break;
      case 3: COLS_FWD(3) break;
      case 4: COLS_FWD(4) break;
      case 5: COLS_FWD(5) break;
      case 6: COLS_FWD(6) break;
      default: throw Error{SHELFI_ERR_ARG, "unsupported batch size"};
    }
#undef COLS_FWD
#undef COLS_FWD1
    SHELFI_HIP(hipGetLastError());
  }
}

}  // namespace shelfi
