// gram.hip — the Gram matrix of C encrypted batches on gfx950: out[p(i, j)] = EvalInnerProduct(u_i, u_j) for
// every i <= j, the upper triangle row-major (p(i, j) = i C - i (i - 1) / 2 + (j - i)), bit for bit what
// dot.hip gives pair by pair, with the inputs read once per TILE of pairs and ONE batched key switch:
//
//   gram_partial_kernel      a workgroup owns a tile of 2 x 2 learners (kGramTile): it loads each of its
//                            learners' ciphertexts once per k and updates every pair of the tile from
//                            registers -> canonical partial sums, one set per slice of the K ciphertexts
//   gram_reduce_intt_kernel  dot_reduce_block once per pair: c0, c1 -> the key switch's output batch, c2 ->
//                            d2e / d2c at the pair's place in the batch ks_scratch_layout describes
//   launch_key_switch        keyswitch.hip's, unchanged, over the chain's pairs
//
// A chain is a run of whole tiles (row-major over tile rows and columns).  The one chain of a call that fits
// its budget indexes its pairs by p itself and switches keys in `out`; a chain of fewer tiles numbers its
// pairs tile by tile, switches keys in the first slice of the partials (folded in place) and copies the
// results to their places in `out` (gram_scatter_kernel).  Sums mod q_t are exact: no output bit depends on
// the tiling, the slice count or the chains.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "dot_dev.h"
#include "shelfi_internal.h"

namespace shelfi {

constexpr int kGramMaxTiles = (kGramMaxLearners / kGramTile) * (kGramMaxLearners / kGramTile + 1) / 2;
static_assert(kGramTile == 2, "the slot order of a diagonal tile and the four launched shapes are those of 2 x 2 tiles");

// Learners [i0, i0 + ni) against [j0, j0 + nj), i0 <= j0; i0 == j0 is a diagonal tile (ni == nj): the
// pairs a <= b of its own learners.  base: the chain-local index of the tile's first pair.
struct GramTile {
  uint8_t i0, j0, ni, nj;
  uint32_t base;
};
// By value in the kernel arguments (the learners' base pointers and the chain's tiles: 1.4 KB).
struct GramArgs {
  const uint64_t* u[kGramMaxLearners];
  GramTile tile[kGramMaxTiles];
  uint32_t C;
  uint32_t direct;  // the chain is the whole call: a pair's index in the chain is p(i, j)
};

// index of the pair (i, j), i <= j, in the upper triangle of an n x n matrix, row-major
__host__ __device__ __forceinline__ uint32_t gram_pair_index(uint32_t i, uint32_t j, uint32_t n) {
  return i * n - i * (i - 1) / 2 + (j - i);
}
__host__ __device__ __forceinline__ uint32_t gram_tile_pairs(const GramTile& t) {
  return t.i0 == t.j0 ? t.ni * (t.ni + 1u) / 2 : (uint32_t)t.ni * t.nj;
}
// the chain-local index of the tile's pair (a, b): learners (i0 + a, j0 + b)
__device__ __forceinline__ uint32_t gram_local(const GramTile& t, uint32_t a, uint32_t b, uint32_t C,
                                               uint32_t direct) {
  if (direct) return gram_pair_index(t.i0 + a, t.j0 + b, C);
  return t.base + (t.i0 == t.j0 ? gram_pair_index(a, b, t.ni) : a * t.nj + b);
}
// the pair (a, b) of the tile's slot-th pair, in the order gram_local numbers them
__device__ __forceinline__ void gram_slot_pair(const GramTile& t, uint32_t slot, uint32_t* a, uint32_t* b) {
  if (t.i0 == t.j0) {  // n <= 2: (0, 0), (0, 1), (1, 1)
    *a = slot >> 1;
    *b = (slot + 1) >> 1;
  } else {
    *a = slot / t.nj;
    *b = slot % t.nj;
  }
}

// One tile, one slice, one tower, 2 adjacent coefficients a thread (dot_partial_kernel's arrangement: the
// tower is block-uniform, 16-byte non-temporal loads, 128-bit accumulators folded every dot_fold_interval
// ciphertexts and at the end).  NI x NJ pairs of row learners A against column learners B, or (DIAG) the
// NI (NI + 1) / 2 pairs of A with itself, the squared form on the diagonal.  U ciphertexts of every
// learner are loaded before any is used.
template <int NI, int NJ, bool DIAG>
__device__ __forceinline__ void gram_tile(const uint64_t* (&A)[NI], const uint64_t* (&B)[NJ],
                                          const uint32_t (&dst)[DIAG ? NI * (NI + 1) / 2 : NI * NJ], uint64_t k0, uint64_t k1, uint64_t poly,
                                          uint64_t off, const TowerConst& c, uint64_t* __restrict__ p01,
                                          uint64_t* __restrict__ p2) {
  // one ciphertext a step wherever two learners are held (8, 6 or 4 loads in flight a thread); two a step
  // take the full tiles past 256 registers (DESIGN.md §2.15's table).  One learner: dot's squared path.
  constexpr int U = NI == 1 ? 4 : 1;
  constexpr int NP = DIAG ? NI * (NI + 1) / 2 : NI * NJ;
  const uint64_t ctw = 2 * poly;
  const uint64_t G = dot_fold_interval(c.q);
  du128 acc[NP][3][2];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int m = 0; m < 3; ++m) acc[p][m][0] = acc[p][m][1] = 0;
  // x = (x0, x1), y = (y0, y1): one ciphertext of each learner of pair p
  const auto take = [&](int p, const ulonglong2& x0, const ulonglong2& x1, const ulonglong2& y0,
                        const ulonglong2& y1, bool square) {
    acc[p][0][0] += (du128)x0.x * y0.x;
    acc[p][0][1] += (du128)x0.y * y0.y;
    acc[p][2][0] += (du128)x1.x * y1.x;
    acc[p][2][1] += (du128)x1.y * y1.y;
    if (square) {
      const du128 mx = (du128)x0.x * x1.x, my = (du128)x0.y * x1.y;
      acc[p][1][0] += mx + mx;
      acc[p][1][1] += my + my;
    } else {
      acc[p][1][0] += (du128)x0.x * y1.x;
      acc[p][1][0] += (du128)x1.x * y0.x;
      acc[p][1][1] += (du128)x0.y * y1.y;
      acc[p][1][1] += (du128)x1.y * y0.y;
    }
  };
  const auto step = [&](uint64_t k, auto n) {
    constexpr int V = decltype(n)::value;
    ulonglong2 a[V][NI][2], b[V][DIAG ? 1 : NJ][2];
#pragma unroll
    for (int u = 0; u < V; ++u) {
      const uint64_t i = (k + u) * ctw + off;
#pragma unroll
      for (int l = 0; l < NI; ++l) {
        a[u][l][0] = ld_pair(A[l] + i);
        a[u][l][1] = ld_pair(A[l] + i + poly);
      }
      if constexpr (!DIAG) {
#pragma unroll
        for (int l = 0; l < NJ; ++l) {
          b[u][l][0] = ld_pair(B[l] + i);
          b[u][l][1] = ld_pair(B[l] + i + poly);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < V; ++u) {
      if constexpr (DIAG) {
        int p = 0;
#pragma unroll
        for (int x = 0; x < NI; ++x)
#pragma unroll
          for (int y = x; y < NI; ++y, ++p) take(p, a[u][x][0], a[u][x][1], a[u][y][0], a[u][y][1], x == y);
      } else {
#pragma unroll
        for (int x = 0; x < NI; ++x)
#pragma unroll
          for (int y = 0; y < NJ; ++y) take(x * NJ + y, a[u][x][0], a[u][x][1], b[u][y][0], b[u][y][1], false);
      }
    }
  };
  uint64_t k = k0;
  while (k < k1) {
    const uint64_t ke = min(k1, k + G);
    for (; k + U <= ke; k += U) step(k, std::integral_constant<int, U>());
    for (; k < ke; ++k) step(k, std::integral_constant<int, 1>());
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        acc[p][m][0] = dot_red128(acc[p][m][0], c);
        acc[p][m][1] = dot_red128(acc[p][m][1], c);
      }
  }
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    uint64_t* o = p01 + (uint64_t)dst[p] * ctw + off;
    *reinterpret_cast<ulonglong2*>(o) = make_ulonglong2((uint64_t)acc[p][0][0], (uint64_t)acc[p][0][1]);
    *reinterpret_cast<ulonglong2*>(o + poly) = make_ulonglong2((uint64_t)acc[p][1][0], (uint64_t)acc[p][1][1]);
    *reinterpret_cast<ulonglong2*>(p2 + (uint64_t)dst[p] * poly + off) =
        make_ulonglong2((uint64_t)acc[p][2][0], (uint64_t)acc[p][2][1]);
  }
}

// Grid (512-coefficient block, tower, tile x slice) over the chain's tiles [tile0, tile0 + gridDim.z / S) of
// one shape: full off-diagonal <2, 2, false>, the last column of an odd C <2, 1, false>, diagonal <2, 2, true>,
// and the one-learner diagonal tile of an odd C <1, 1, true> (dot's squared path).  A narrower instance runs
// the same sums on fewer pairs, so ragged edges give the same bits.  The partials of a chain of kc pairs: the
// c0, c1 sums p01 [S][kc][2][Ll][N], then the c2 sums p2 [S][kc][Ll][N], so that one slice of p01 is a batch
// of kc two-component ciphertexts.
template <int NI, int NJ, bool DIAG>
__global__ __launch_bounds__(256) void gram_partial_kernel(const GramArgs g, uint32_t tile0, uint64_t K, uint32_t S,
                                                           uint32_t kc, uint32_t Ll, uint32_t logN,
                                                           const TowerConst* __restrict__ tq,
                                                           uint64_t* __restrict__ part) {
  const uint32_t t = blockIdx.y, s = blockIdx.z % S;
  const GramTile tl = g.tile[tile0 + blockIdx.z / S];
  const TowerConst c = tq[t];
  const uint64_t k0 = (uint64_t)s * K / S, k1 = (uint64_t)(s + 1) * K / S;  // balanced: no empty slice (S <= K)
  const uint64_t poly = (uint64_t)Ll << logN;
  const uint64_t off = ((uint64_t)t << logN) + (uint64_t)blockIdx.x * 512 + 2u * threadIdx.x;
  const uint64_t* A[NI];
  const uint64_t* B[NJ];
#pragma unroll
  for (int l = 0; l < NI; ++l) A[l] = g.u[tl.i0 + l];
#pragma unroll
  for (int l = 0; l < NJ; ++l) B[l] = g.u[tl.j0 + l];
  constexpr int NP = DIAG ? NI * (NI + 1) / 2 : NI * NJ;
  uint32_t dst[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    uint32_t a, b;
    gram_slot_pair(tl, i, &a, &b);
    dst[i] = gram_local(tl, a, b, g.C, g.direct);
  }
  gram_tile<NI, NJ, DIAG>(A, B, dst, k0, k1, poly, off, c, part + (uint64_t)s * kc * 2 * poly,
                          part + ((uint64_t)S * kc * 2 + (uint64_t)s * kc) * poly);
}

// Grid ((tower, NTT block), pair slot of a tile, tile): dot_reduce_block on the slot's pair.  c0, c1 go to
// the key switch's output batch: `out` (a direct chain), or the pair's own words of the first slice of p01,
// which this workgroup alone reads and writes.
__global__ __launch_bounds__(256) void gram_reduce_intt_kernel(const GramArgs g, uint64_t* part, uint32_t S,
                                                               uint32_t kc, uint32_t Ll, uint32_t logN,
                                                               uint32_t blkLog, const uint64_t* __restrict__ itw,
                                                               const uint64_t* __restrict__ itwp,
                                                               const TowerConst* __restrict__ tq, uint64_t* out,
                                                               uint64_t* __restrict__ d2e,
                                                               uint64_t* __restrict__ d2c) {
  extern __shared__ __attribute__((aligned(16))) uint64_t sm[];
  const GramTile tl = g.tile[blockIdx.z];
  if (blockIdx.y >= gram_tile_pairs(tl)) return;
  uint32_t pa, pb;
  gram_slot_pair(tl, blockIdx.y, &pa, &pb);
  const uint64_t lp = gram_local(tl, pa, pb, g.C, g.direct);
  const uint32_t sh = logN - blkLog;
  const uint32_t t = blockIdx.x >> sh, b = blockIdx.x & ((1u << sh) - 1);
  const uint64_t poly = (uint64_t)Ll << logN;
  const uint64_t* p01 = part + lp * 2 * poly;
  const uint64_t* p2 = part + ((uint64_t)S * kc * 2 + lp) * poly;
  uint64_t* o = (g.direct ? out : part) + lp * 2 * poly;
  dot_reduce_block(sm, p01, p01 + poly, (uint64_t)kc * 2 * poly, p2, (uint64_t)kc * poly, S, t, b, logN, blkLog, itw,
                   itwp, tq[t], o, o + poly, d2e + lp * poly, d2c + lp * poly);
}

// Grid (512-word block of a ciphertext, pair slot, tile): a chain of fewer tiles than the call's copies its
// key-switched pairs from the batch to their places in out.
__global__ __launch_bounds__(256) void gram_scatter_kernel(const GramArgs g, const uint64_t* __restrict__ batch,
                                                           uint64_t ctw, uint64_t* __restrict__ out) {
  const GramTile tl = g.tile[blockIdx.z];
  if (blockIdx.y >= gram_tile_pairs(tl)) return;
  uint32_t pa, pb;
  gram_slot_pair(tl, blockIdx.y, &pa, &pb);
  const uint64_t e = (uint64_t)blockIdx.x * 512 + 2u * threadIdx.x;
  const uint64_t from = gram_local(tl, pa, pb, g.C, 0) * ctw + e;
  const uint64_t to = gram_pair_index(tl.i0 + pa, tl.j0 + pb, g.C) * ctw + e;
  *reinterpret_cast<ulonglong2*>(out + to) = *reinterpret_cast<const ulonglong2*>(batch + from);
}

uint64_t gram_pairs(uint64_t C) { return C * (C + 1) / 2; }
uint64_t gram_tiles(uint64_t C) { return gram_pairs((C + kGramTile - 1) / kGramTile); }

// Slices of the K ciphertexts: dot's ceil(K / slice_cts), at most kDotMaxSlices, but no more than bring the
// call's workgroups (tiles x towers x 512-coefficient blocks) to kGramFillGroups.
uint32_t gram_slices(uint64_t C, uint64_t K, uint32_t Ll, uint32_t logN, uint64_t slice_cts) {
  const uint64_t groups = gram_tiles(C) * Ll << (logN > 9 ? logN - 9 : 0);
  const uint64_t fill = (kGramFillGroups + groups - 1) / groups;
  const uint64_t per = std::max<uint64_t>(1, slice_cts);
  return (uint32_t)std::min<uint64_t>({(uint64_t)kDotMaxSlices, fill, K / per + (K % per ? 1 : 0)});
}

// scratch: the key switch's for kc ciphertexts (rounded up to 64 bytes) | the partials [S][kc][3][Ll][N]
static size_t gram_ks_bytes(const KsArgs& a, uint64_t kc) {
  return (ks_scratch_bytes(a.Ll, a.kP, a.dn, a.alpha, 1u << a.logN, kc) + 63) & ~(size_t)63;
}
size_t gram_scratch_bytes(const KsArgs& a, uint32_t S, uint64_t kc) {
  return gram_ks_bytes(a, kc) + ((size_t)S * kc * 3 * a.Ll << a.logN) * 8;
}

void launch_gram(const KsArgs& a, const DeviceTables& dtq, const DeviceTables& dte, const DeviceTables* dtf,
                 const uint64_t* evk, const uint64_t* evk_sh, const uint64_t* const* u, uint32_t C, uint64_t t0,
                 uint64_t tc, uint64_t K, uint32_t S, uint64_t* out, void* scratch, hipStream_t s) {
  if (!K || !tc) return;
  if (a.logN < 9) throw Error{SHELFI_ERR_ARG, "Gram: unsupported ring dimension"};
  if (S < 1 || S > (uint32_t)kDotMaxSlices || S > K) throw Error{SHELFI_ERR_ARG, "Gram: bad slice count"};
  if (C < 1 || C > (uint32_t)kGramMaxLearners || t0 + tc > gram_tiles(C)) throw Error{SHELFI_ERR_ARG, "Gram: bad tile range"};
  GramArgs g{};
  for (uint32_t i = 0; i < C; ++i) g.u[i] = u[i];
  g.C = C;
  g.direct = tc == gram_tiles(C);
  // the chain's tiles grouped by shape (a launch each); a tile's pairs are numbered in the tiles' own order
  const auto shape_of = [](const GramTile& tl) { return tl.i0 == tl.j0 ? (tl.ni == 2 ? 2 : 3) : (tl.nj == 2 ? 0 : 1); };
  uint32_t kc = 0, first[5] = {};
  for (int pass = 0; pass < 2; ++pass) {  // count the shapes, then place the tiles
    uint32_t at[4] = {first[0], first[1], first[2], first[3]};
    uint64_t ti = 0;  // tiles in row-major order; the chain takes [t0, t0 + tc)
    for (uint32_t i0 = 0; i0 < C; i0 += kGramTile)
      for (uint32_t j0 = i0; j0 < C; j0 += kGramTile, ++ti) {
        if (ti < t0 || ti >= t0 + tc) continue;
        GramTile tl;
        tl.i0 = (uint8_t)i0, tl.j0 = (uint8_t)j0;
        tl.ni = (uint8_t)std::min<uint32_t>(kGramTile, C - i0), tl.nj = (uint8_t)std::min<uint32_t>(kGramTile, C - j0);
        const int sp = shape_of(tl);
        if (!pass) {
          ++first[sp + 1];
          continue;
        }
        tl.base = kc;
        kc += gram_tile_pairs(tl);
        g.tile[at[sp]++] = tl;
      }
    if (!pass)
      for (int sp = 0; sp < 4; ++sp) first[sp + 1] += first[sp];
  }
  uint64_t* part = reinterpret_cast<uint64_t*>(static_cast<char*>(scratch) + gram_ks_bytes(a, kc));
  const auto partial = [&](auto kernel, int sp) {
    const uint32_t n = first[sp + 1] - first[sp];
    if (!n) return;
    hipLaunchKernelGGL(kernel, dim3(1u << (a.logN - 9), a.Ll, n * S), dim3(256), 0, s, g, first[sp], K, S, kc, a.Ll,
                       a.logN, a.tq, part);
    SHELFI_HIP(hipGetLastError());
  };
  partial(gram_partial_kernel<2, 2, false>, 0);
  partial(gram_partial_kernel<2, 1, false>, 1);
  partial(gram_partial_kernel<2, 2, true>, 2);
  partial(gram_partial_kernel<1, 1, true>, 3);
  const uint32_t blkLog = ntt_block_log(a.logN), sh = a.logN - blkLog;
  const KsScratch ks = ks_scratch_layout(a, kc, scratch);
  constexpr uint32_t slots = kGramTile * kGramTile;
  hipLaunchKernelGGL(gram_reduce_intt_kernel, dim3(a.Ll << sh, slots, (uint32_t)tc), dim3(256),
                     sizeof(uint64_t) << blkLog, s, g, part, S, kc, a.Ll, a.logN, blkLog, dtq.ipsi_rev, dtq.ipsi_rev_sh,
                     a.tq, out, ks.d2e, ks.d2c);
  SHELFI_HIP(hipGetLastError());
  launch_key_switch(a, dtq, dte, dtf, evk, evk_sh, kc, g.direct ? out : part, scratch, s);
  if (g.direct) return;
  const uint64_t ctw = 2ull * a.Ll << a.logN;
  hipLaunchKernelGGL(gram_scatter_kernel, dim3((uint32_t)(ctw / 512), slots, (uint32_t)tc), dim3(256), 0, s, g, part, ctw,
                     out);
  SHELFI_HIP(hipGetLastError());
}

}  // namespace shelfi
