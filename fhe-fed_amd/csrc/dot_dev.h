// dot_dev.h — device code shared by the summed-tensor calls (dot.hip: EvalInnerProduct; gram.hip: the Gram
// matrix): the 128-bit accumulator's reduction and fold interval, the 16-byte streaming load, and the pass
// that sums the slices' partial tensors of one result and hands its c2 to the key switch.
#pragma once

#include "dev_common.h"

namespace shelfi {

typedef unsigned __int128 du128;

// acc (ANY 128-bit value) -> [0, q): acc = hi 2^64 + lo; shoup_mul reduces hi r64 for any 64-bit hi
// (r64 = 2^64 mod q < q with its Shoup companion: x w - floor(x w' / 2^64) q < 2q for every x < 2^64),
// red64 reduces any 64-bit lo, and addmod joins two canonical residues.  keyswitch.hip's red128 is
// this same arithmetic; its "< 2^124" comment describes its callers' sums, not a limit of the
// reduction.  Restated here so that the fold interval below rests on a statement made in this file.
__device__ __forceinline__ uint64_t dot_red128(du128 acc, const TowerConst& c) {
  const uint64_t hi = (uint64_t)(acc >> 64), lo = (uint64_t)acc;
  return addmod(shoup_mul(hi, c.r64, c.r64_shoup, c.q), red64(lo, c.q, c.one_shoup), c.q);
}

// Fold interval G, in ciphertexts, for a tower of b = bitlength(q) bits.  The reduction takes any
// 128-bit value, so the only limit is that the accumulator itself must not wrap.  An accumulator
// starts a run at r < q (the previous fold's residue, carried in the accumulator) and takes P
// products of canonical residues, each <= (q - 1)^2 <= (2^b - 2)^2 = 2^2b - 2^(b+2) + 4:
//   r + P (q - 1)^2  <  2^b + 2^(e+2b) - 2^(e+b+2) + 2^(e+2)        with P = 2^e
// With e = 128 - 2b that is 2^128 - (2^(130-b) - 2^(130-2b) - 2^b) < 2^128 whenever
// 2^b + 2^(130-2b) <= 2^(130-b), true for 44 <= b <= 63; with e capped at 32 (b < 48) the sum stays
// below 2^(33+2b) < 2^128.  c1 takes two products per ciphertext (the squared path doubles one), c0
// and c2 one, so a run may hold G = P / 2 ciphertexts: 128 on a 60-bit tower, 2^31 from 48 bits down.
// The bound is one accumulator's: it holds for each of a Gram tile's accumulators as it does for dot's.
__device__ __forceinline__ uint64_t dot_fold_interval(uint64_t q) {
  const int b = 64 - __builtin_clzll(q);
  const int e = max(min(128 - 2 * b, 32), 1);  // (b <= 60 in every chain the library builds)
  return 1ull << (e - 1);
}

__device__ __forceinline__ ulonglong2 ld_pair(const uint64_t* p) {
  const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
  return make_ulonglong2(((uint64_t)v.y << 32) | v.x, ((uint64_t)v.w << 32) | v.z);
}

// One workgroup's share, NTT block b of tower t (c = that tower's constants), of the pass between the partial
// sums and the key switch: the S <= 16 canonical partials of every residue (p0, p1, p2: the first slice's
// three component sums of this result; ss01 words from slice to slice of p0 and p1, ss2 of p2) are summed as
// plain uint64 (16 q < 2^64 for q < 2^60: the argument of threshold fusion and mk_key_add_kernel) and folded
// by one red64; c0 and c1 go to out0 / out1, c2 to d2e (EVALUATION) and into LDS, where the first inverse
// stages run into d2c.  All pointers are the result's own polynomials [Ll][N].  out0 / out1 may be p0 / p1
// themselves: a thread writes only the residues it has read.
__device__ __forceinline__ void dot_reduce_block(uint64_t* sm, const uint64_t* p0, const uint64_t* p1, uint64_t ss01,
                                                 const uint64_t* __restrict__ p2, uint64_t ss2, uint32_t S,
                                                 uint32_t t, uint32_t b, uint32_t logN, uint32_t blkLog,
                                                 const uint64_t* __restrict__ itw,
                                                 const uint64_t* __restrict__ itwp, const TowerConst& c,
                                                 uint64_t* out0, uint64_t* out1, uint64_t* __restrict__ d2e,
                                                 uint64_t* __restrict__ d2c) {
  const uint32_t N = 1u << logN, blk = 1u << blkLog;
  const uint64_t q = c.q, osh = c.one_shoup;
  const uint64_t off = ((uint64_t)t << logN) + ((uint64_t)b << blkLog);
  const ulonglong2* P0 = reinterpret_cast<const ulonglong2*>(p0 + off);
  const ulonglong2* P1 = reinterpret_cast<const ulonglong2*>(p1 + off);
  const ulonglong2* P2 = reinterpret_cast<const ulonglong2*>(p2 + off);
  ss01 /= 2, ss2 /= 2;  // in 16-byte pairs
  ulonglong2* O0 = reinterpret_cast<ulonglong2*>(out0 + off);
  ulonglong2* O1 = reinterpret_cast<ulonglong2*>(out1 + off);
  ulonglong2* E2 = reinterpret_cast<ulonglong2*>(d2e + off);
  for (uint32_t p = threadIdx.x; p < blk / 2; p += 256) {
    ulonglong2 r0 = make_ulonglong2(0, 0), r1 = r0, r2 = r0;
    for (uint32_t s = 0; s < S; ++s) {
      const ulonglong2 v0 = P0[s * ss01 + p], v1 = P1[s * ss01 + p], v2 = P2[s * ss2 + p];
      r0.x += v0.x;
      r0.y += v0.y;
      r1.x += v1.x;
      r1.y += v1.y;
      r2.x += v2.x;
      r2.y += v2.y;
    }
    r0 = make_ulonglong2(red64(r0.x, q, osh), red64(r0.y, q, osh));
    r1 = make_ulonglong2(red64(r1.x, q, osh), red64(r1.y, q, osh));
    r2 = make_ulonglong2(red64(r2.x, q, osh), red64(r2.y, q, osh));
    O0[p] = r0;
    O1[p] = r1;
    E2[p] = r2;
    lds_put2(sm, p, r2);
  }
  __syncthreads();
  ks_intt_block_out(sm, blkLog, b, logN, itw + (uint64_t)t * N, itwp + (uint64_t)t * N, c, d2c + off);
}

}  // namespace shelfi
