// transform_dev.h — device code shared by ntt.hip, encrypt.hip and decrypt.hip: the block order
// of the NTT block passes, the inverse chunk pass, the generic inverse blocks kernel, the range
// flag's store, and the special FFT's register chunks and whole-vector exchanges.
#pragma once

#include <type_traits>

#include "dev_common.h"

namespace shelfi {

// XCD-aware block order for the block passes.  Blocks b and b + 8 share an XCD (observed
// round-robin dealing, MI355X_MICROARCH "Workgroup dispatch"; used for speed only: any
// placement gives the same results).  The G = L 2^sstart (tower, block) combos each own a
// shared slice of twiddles and key words (64-160 KiB per workgroup, 4-6 MiB per launch at
// 2^15/L4, more than one XCD's 4 MiB L2); dealt in natural order every XCD touches all of
// them and they stream from the Infinity Cache.  With xg = G (G % 8 == 0) XCD slot x = bid % 8
// owns combos [x G/8, (x+1) G/8) for every ciphertext, 1/8 of the slices.  Returns the
// logical block id k G + combo; xg == 0 keeps the natural order.
__device__ __forceinline__ uint32_t xcd_block(uint32_t bid, uint32_t xg) {
  if (!xg) return bid;
  const uint32_t g8 = xg >> 3, i = bid >> 3;
  const uint32_t k = i / g8;
  return k * xg + (bid & 7) * g8 + (i - k * g8);
}

// Inverse (GS) chunk of KC stages starting at local half-size 2^T0: set s -> g = s >> T0,
// j0 = g 2^(T0+KC) + (s mod 2^T0), elements j0 + m 2^T0; stage-i twiddles are
// tb[2^l + g 2^(KC-1-i) + gs], gs < 2^(KC-1-i), l = BL - 1 - T0 - i.
template <int BL, int T0, int KC, bool IN8, class Load, class Store>
__device__ __forceinline__ void inv_chunk_ct(const ulonglong2* __restrict__ tb, uint64_t q,
                                             uint64_t n8q, Load ld, Store st) {
  constexpr int M = 1 << KC, NS = (1 << (BL - KC)) / 256;
  static_assert(NS >= 1, "chunk plan");
#pragma unroll
  for (int r = 0; r < NS; ++r) {
    const uint32_t s = threadIdx.x + 256u * r;
    const uint32_t g = s >> T0;
    const uint32_t j0 = (g << (T0 + KC)) + (s & ((1u << T0) - 1));
    const uint32_t pj0 = lpad(j0);
    uint64_t x[M];
#pragma unroll
    for (int m = 0; m < M; ++m) x[m] = ld(j0 + (m << T0), pj0 + lofs<(1 << T0)>(m));
#pragma unroll
    for (int i = 0; i < KC; ++i) {
      const int hm = 1 << i;
      const ulonglong2* __restrict__ tw = tb + (1u << (BL - 1 - T0 - i)) + (g << (KC - 1 - i));
#pragma unroll
      for (int gs = 0; gs < (M >> (i + 1)); ++gs) {
        const ulonglong2 W = tw[gs];
#pragma unroll
        for (int mm = 0; mm < hm; ++mm) {
          if (gs_in8<IN8>(i, mm))
            gs_bfly_b<true>(x[gs * 2 * hm + mm], x[gs * 2 * hm + mm + hm], W.x, W.y, q, n8q);
          else
            gs_bfly_b<false>(x[gs * 2 * hm + mm], x[gs * 2 * hm + mm + hm], W.x, W.y, q, n8q);
        }
      }
    }
    st(r, j0, pj0, x);
  }
}

// Inverse blocks pass: small half-sizes first (LDS), then the top LOGR stages on
// register columns (ntt_inv_cols), scaled by N^-1 in the last pass.
// With ct != nullptr the input is decrypt's c0 + c1*s (ckks.cpp:189), formed while
// filling LDS from the ciphertext batch [K][2][L][N] (poly p = k*L + t).
// FZ = FuseIn: the input is the sum of fz.P partial decryptions [K][ctL][N] instead (no key).
template <class FZ = NoFuse>
__global__ __launch_bounds__(256) void ntt_inv_blocks(uint64_t* __restrict__ polys, uint32_t L,
                                                      uint32_t logN, uint32_t blkLog,
                                                      const uint64_t* __restrict__ tw,
                                                      const uint64_t* __restrict__ twp,
                                                      const TowerConst* __restrict__ tcs,
                                                      int scale_ninv,
                                                      const uint64_t* __restrict__ ct,
                                                      const uint64_t* __restrict__ sk,
                                                      const uint64_t* __restrict__ sksh, int sum_in,
                                                      uint32_t ctL, FZ fz) {
  constexpr bool FUSE = std::is_same<FZ, FuseIn>::value;
  extern __shared__ __attribute__((aligned(16))) uint64_t sm[];
  const uint32_t N = 1u << logN, blk = 1u << blkLog;
  const uint32_t sh = logN - blkLog, nb = 1u << sh;
  const uint64_t poly = blockIdx.x >> sh;
  const uint32_t b = blockIdx.x & (nb - 1);
  const uint32_t t = (uint32_t)(poly % L);
  const TowerConst& c = tcs[t];
  const uint64_t q = c.q;
  uint64_t* __restrict__ a = polys + poly * N + ((uint64_t)b << blkLog);
  if constexpr (FUSE) {
    const uint64_t e0 = ((poly / L) * ctL << logN) + ((uint64_t)t << logN) + ((uint64_t)b << blkLog);
    for (uint32_t p = threadIdx.x; p < blk / 2; p += 256) {
      ulonglong2 x = make_ulonglong2(0, 0);
      for (uint32_t i = 0; i < fz.P; ++i) {
        const ulonglong2 y = reinterpret_cast<const ulonglong2*>(fz.part[i] + e0)[p];
        x.x += y.x;
        x.y += y.y;
      }
      lds_put2(sm, p, make_ulonglong2(red64(x.x, q, c.one_shoup), red64(x.y, q, c.one_shoup)));
    }
  } else if (ct) {
    const uint64_t kk = poly / L, off = ((uint64_t)t << logN) + ((uint64_t)b << blkLog);
    const ulonglong2* c0 = reinterpret_cast<const ulonglong2*>(ct + (kk * 2 * ctL << logN) + off);
    const ulonglong2* c1 = reinterpret_cast<const ulonglong2*>(ct + ((kk * 2 + 1) * ctL << logN) + off);
    const ulonglong2* s = reinterpret_cast<const ulonglong2*>(sk + off);
    const ulonglong2* ss = reinterpret_cast<const ulonglong2*>(sksh + off);
    for (uint32_t p = threadIdx.x; p < blk / 2; p += 256) {
      ulonglong2 x0 = c0[p];
      const ulonglong2 x1 = c1[p], sv = s[p], sw = ss[p];
      if (sum_in) x0 = make_ulonglong2(red64(x0.x, q, c.one_shoup), red64(x0.y, q, c.one_shoup));
      lds_put2(sm, p, make_ulonglong2(addmod(x0.x, shoup_mul(x1.x, sv.x, sw.x, q), q),
                                      addmod(x0.y, shoup_mul(x1.y, sv.y, sw.y, q), q)));
    }
  } else {
    for (uint32_t p = threadIdx.x; p < blk / 2; p += 256)
      lds_put2(sm, p, reinterpret_cast<const ulonglong2*>(a)[p]);
  }
  __syncthreads();
  ntt_inv_block_stages(sm, blkLog, b, logN, tw + (uint64_t)t * N, twp + (uint64_t)t * N, q);
  if (scale_ninv) {
    const uint64_t ni = c.ninv, nip = c.ninv_shoup;
    for (uint32_t p = threadIdx.x; p < blk / 2; p += 256) {
      const ulonglong2 v = lds_get2(sm, p);
      reinterpret_cast<ulonglong2*>(a)[p] = make_ulonglong2(canon4(shoup_lazy(v.x, ni, nip, q), q),
                                                            canon4(shoup_lazy(v.y, ni, nip, q), q));
    }
  } else {  // lazy values in [0, 4q): the columns pass canonicalises
    for (uint32_t p = threadIdx.x; p < blk / 2; p += 256)
      reinterpret_cast<ulonglong2*>(a)[p] = lds_get2(sm, p);
  }
}

// The NoFuse form has one instance, emitted by ntt.hip; launch_decrypt launches that one.
extern template __global__ void ntt_inv_blocks<NoFuse>(uint64_t*, uint32_t, uint32_t, uint32_t, const uint64_t*,
                                                       const uint64_t*, const TowerConst*, int, const uint64_t*,
                                                       const uint64_t*, const uint64_t*, int, uint32_t, NoFuse);

// Raises word `word` of a GenFlag (shelfi_internal.h) with the call's generation.
__device__ __forceinline__ void gen_flag_set(GenFlag f, int word) {
  __hip_atomic_store(f.p + word, f.gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Compile-time forms of the FFT block passes (round 3): the same butterflies, in the same order
// per element, as fft_fwd_blocks / fft_inv_blocks, but run as register chunks of 2^KC
// elements (a set j0 + m 2^A, m < 2^KC, covers the stages of half-size 2^A .. 2^(A+KC-1)) with
// the LDS block exchanged only between chunks: 3 barriers instead of 10-11, the first chunk
// loaded and the last chunk stored straight from registers.  Bit-identical outputs.
template <int KC, int A>
__device__ __forceinline__ void fft_dit_set(double2 (&v)[1 << KC], uint32_t l, const double2* __restrict__ tw) {
#pragma unroll
  for (int i = 0; i < KC; ++i) {  // half-size 2^(A+i), ascending (DIT)
#pragma unroll
    for (int m0 = 0; m0 < (1 << KC); ++m0) {
      if (m0 & (1 << i)) continue;
      const int m1 = m0 + (1 << i);
      const double2 W = tw[(1u << (A + i)) + l + ((uint32_t)(m0 & ((1 << i) - 1)) << A)];
      const double2 u = v[m0];
      const double2 w = cmul(v[m1], W);
      v[m0] = cadd(u, w);
      v[m1] = csub(u, w);
    }
  }
}
template <int KC, int A>
__device__ __forceinline__ void fft_dif_set(double2 (&v)[1 << KC], uint32_t l, const double2* __restrict__ tw) {
#pragma unroll
  for (int i = KC - 1; i >= 0; --i) {  // half-size 2^(A+i), descending (DIF)
#pragma unroll
    for (int m0 = 0; m0 < (1 << KC); ++m0) {
      if (m0 & (1 << i)) continue;
      const int m1 = m0 + (1 << i);
      const double2 W = tw[(1u << (A + i)) + l + ((uint32_t)(m0 & ((1 << i) - 1)) << A)];
      const double2 a0 = v[m0], a1 = v[m1];
      v[m0] = cadd(a0, a1);
      v[m1] = cmul(csub(a0, a1), W);
    }
  }
}
// One chunk over all 2^(BL-KC) sets of a block, 2^(BL-3) threads: ld(j) / st(j, v) take block
// offsets.
template <int BL, int KC, int A, bool DIT, class Load, class Store>
__device__ __forceinline__ void fft_chunk(const double2* __restrict__ tw, Load ld, Store st) {
  constexpr int T = 1 << (BL - 3), NS = (1 << (BL - KC)) / T;
  static_assert(NS >= 1, "chunk plan");
#pragma unroll
  for (int r = 0; r < NS; ++r) {
    const uint32_t s = threadIdx.x + (uint32_t)T * r;
    const uint32_t l = s & ((1u << A) - 1), j0 = ((s >> A) << (A + KC)) | l;
    double2 v[1 << KC];
#pragma unroll
    for (int m = 0; m < (1 << KC); ++m) v[m] = ld(j0 + ((uint32_t)m << A));
    if (DIT)
      fft_dit_set<KC, A>(v, l, tw);
    else
      fft_dif_set<KC, A>(v, l, tw);
#pragma unroll
    for (int m = 0; m < (1 << KC); ++m) st(j0 + ((uint32_t)m << A), v[m]);
  }
}
// The LDS block of the FFT chunk passes is XOR-swizzled (round 4): element j lives at
// j ^ ((j >> 3) & 15), a bijection of every aligned 128-element group.  A chunk at stride 2^A hands
// lane l the elements j0(l) + m 2^A; with A = 0 (the DIT pass's first chunk, 8 consecutive elements
// per lane) every lane of a ds_write_b128 group hit the same 16-B slot mod 128 B (8-way), and the
// DIF pass's A = 2 and A = 0 chunks hit 4 slots per 16-lane ds_read_b128 group.  Counted per
// instruction by a model of the chunk addresses and the gfx950 lane groups (MI355X_MICROARCH.md
// §LDS), which reproduces the measured SQ_LDS_BANK_CONFLICT / SQ_INSTS_LDS of round 3 exactly
// (10.0 for fft_fwd_blocks_ct<10,...>, 5.33 for fft_inv_blocks_ct<10,...>): swizzled, 0 and 1.33
// (the DIF A = 2 chunk's stores keep a 2-way conflict), and 0 for both BL = 11 passes.
template <bool SWZ = true>
__device__ __forceinline__ uint32_t fft_swz(uint32_t j) { return SWZ ? j ^ ((j >> 3) & 15u) : j; }

// Whole-vector FFT passes (round 5): one 1024-thread workgroup per ciphertext at 2^14 slots holds the
// vector in registers (16 complex values per thread), so the columns and blocks passes share one
// launch and the [K][S] intermediate never goes through HBM (encode: 1.18 -> 0.39 MB per ciphertext;
// decode: 0.92 -> 0.39).  The same butterflies on the same operands as fft_inv_cols<4> +
// fft_inv_blocks_ct<10, ...> (fft_fwd_blocks_ct<10, ...> + fft_fwd_cols<4>): bit-identical outputs.
// Rows <-> blocks go through LDS one component at a time (16 x 1088 doubles = 136 KiB, one workgroup
// per CU); inside a block, a wave exchanges its own 1024 elements (8 KiB) with no workgroup barrier.
// LDS layouts.  Padded rows (not an XOR swizzle) keep each thread's 16 addresses at compile-time offsets
// from one base: an XOR swizzle's 32 live addresses spilled under the 128-VGPR cap of 1024-thread
// workgroups.  Each exchange has its own padding, chosen with a model of the ds_read_b64 (2 x 32 lanes, 64
// banks) and ds_write_b64 / read2 (4 x 16 lanes, 32 banks) groups of MI355X_MICROARCH.md §LDS so that both
// of its access shapes are conflict-free (one shared padding left 2-way conflicts: SQ_LDS_BANK_CONFLICT 3.4
// cycles per LDS instruction in fft_inv_whole, profiles/r05p):
//   blocks <-> rows transposes and the flooding statistics, e + (e >> 5)   (fft_wpad, fft_wt1, fft_wx3)
//   exchanges between 4 s + m and 64 (s >> 2) + (s & 3) + 4 m, e + (e >> 4)     (fft_xa1, fft_xa2)
//   exchanges between 64 (s >> 2) + (s & 3) + 4 m and s + 64 m, e + 2 (e >> 5)  (fft_xb2, fft_xb3)
// The closed forms below are those paddings of the set shapes 4 (l + 64 q) + r (m = 4 q + r),
// 64 (l >> 2) + (l & 3) + 4 m and l + 64 m, for lane l and register m.
constexpr uint32_t kFftWholeLogS = 14;
// One 1024-thread workgroup per vector fills the chip only for batches of hundreds of ciphertexts: below
// kFftWholeMinK the multi-pass FFTs (many workgroups per vector) are faster -- at K = 4 / 16 / 64 encrypt
// 21.3 / 6.9 / 3.70 vs 24.9 / 7.7 / 3.73 us/ct, decrypt 10.5 / 3.5 / 1.53 vs 13.7 / 4.2 / 1.64; at K = 256
// the whole-vector kernels win, 2.93 vs 2.97 and 0.99 vs 1.03 (profiles/r05zc/small_k.txt)
constexpr uint64_t kFftWholeMinK = 128;
constexpr uint32_t kFftWholeRow = 1088;  // doubles per 1024-element block slice (the largest padding, 1087)
__device__ __forceinline__ uint32_t fft_wpad(uint32_t e) { return e + (e >> 5); }
__device__ __forceinline__ uint32_t fft_wt1(uint32_t l, int m) { return 4 * l + (l >> 3) + 264u * (m >> 2) + (m & 3); }
__device__ __forceinline__ uint32_t fft_wx3(uint32_t l, int m) { return l + (l >> 5) + 66u * m; }
__device__ __forceinline__ uint32_t fft_xa1(uint32_t l, int m) { return 4 * l + (l >> 2) + 272u * (m >> 2) + (m & 3); }
__device__ __forceinline__ uint32_t fft_xa2(uint32_t l, int m) { return 68 * (l >> 2) + (l & 3) + 4u * m + (m >> 2); }
__device__ __forceinline__ uint32_t fft_xb2(uint32_t l, int m) {
  return 68 * (l >> 2) + (l & 3) + 4u * m + 2u * (m >> 3);
}
__device__ __forceinline__ uint32_t fft_xb3(uint32_t l, int m) { return l + 2 * (l >> 5) + 68u * m; }

// A wave's exchange inside its block's 1024 elements: a[m] (at padded block position P(m)) -> a[m] (at
// Q(m)), real parts first, then imaginary parts, through the wave's LDS slice.
template <class PF, class QF>
__device__ __forceinline__ void fft_wave_xch(double2 (&a)[16], double* __restrict__ Ls, PF P, QF Q) {
#pragma unroll
  for (int m = 0; m < 16; ++m) Ls[P(m)] = a[m].x;
  wave_lds_sync();
#pragma unroll
  for (int m = 0; m < 16; ++m) a[m].x = Ls[Q(m)];
  wave_lds_sync();
#pragma unroll
  for (int m = 0; m < 16; ++m) Ls[P(m)] = a[m].y;
  wave_lds_sync();
#pragma unroll
  for (int m = 0; m < 16; ++m) a[m].y = Ls[Q(m)];
  wave_lds_sync();
}

// Rows (thread T holds row r's column T in a[r]) <-> blocks (wave w holds block w's element l + 64 m in
// a[m]) through the workgroup's 16 x 1024-double LDS, one component at a time.  TO_BLOCKS: rows -> blocks.
template <bool TO_BLOCKS>
__device__ __forceinline__ void fft_whole_transpose(double2 (&a)[16], double* __restrict__ lds) {
  const uint32_t T = threadIdx.x, w = T >> 6, l = T & 63;
#pragma unroll
  for (int part = 0; part < 2; ++part) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const double v = part ? a[i].y : a[i].x;
      if (TO_BLOCKS)
        lds[i * kFftWholeRow + fft_wpad(T)] = v;
      else
        lds[w * kFftWholeRow + fft_wx3(l, i)] = v;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const double v = TO_BLOCKS ? lds[w * kFftWholeRow + fft_wx3(l, i)] : lds[i * kFftWholeRow + fft_wpad(T)];
      if (part)
        a[i].y = v;
      else
        a[i].x = v;
    }
    __syncthreads();
  }
}

}  // namespace shelfi
