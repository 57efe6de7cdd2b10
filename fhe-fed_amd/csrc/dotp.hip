// dotp.hip — EvalInnerProduct(ciphertext, plaintext) on gfx950: the projections of C encrypted batches on R
// plaintext batches, out[c R + r] = sum_k u_{c,k} (.) p_{r,k} in both components (PALISADE's
// EvalInnerProduct(ct, pt): EvalMult(ct, pt) + EvalAddMany as one device call).  No key:
//
//   out[c R + r][i] = sum_k u_{c,k,i} p_{r,k}  mod q_t      i = 0, 1, per tower and coefficient, canonical
//
// What remains is a streaming pass, three polynomial reads a (ciphertext, plaintext) pair per tower where
// mult_plain + add move eleven, with the inputs read once per TILE of pairs:
//
//   dotp_partial_kernel  a workgroup owns a tile of NC learners x NR plaintexts: it loads its learners' 2 NC
//                        polynomials and its NR plaintext polynomials once per k and updates the 2 NC NR sums
//                        from registers -> canonical sums, one set per slice of the K ciphertexts; with one
//                        slice they are the result and go straight to out
//   dotp_reduce_kernel   (S > 1) sums the S partial sets pointwise into out
//
// Sums mod q_t are exact: no output bit depends on the tiling, the slice count or the launch geometry.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "dot_dev.h"
#include "shelfi_internal.h"

namespace shelfi {

// the learners' base pointers, by value in the kernel arguments (256 bytes)
struct DotpArgs {
  const uint64_t* u[kDotpMaxBatches];
};

// Fold interval, in ciphertexts, of one of this file's accumulators.  dot_dev.h's argument, restated: the
// reduction (dot_red128) takes any 128-bit value, so the only limit is that the accumulator must not wrap.  It
// starts a run at r < q (the previous fold's residue) and takes P = 2^e products of canonical residues, each
// <= (q - 1)^2 <= (2^b - 2)^2 for a tower of b = bitlength(q) bits:
//   r + P (q - 1)^2  <  2^b + 2^(e+2b) - 2^(e+b+2) + 2^(e+2)
// which with e = 128 - 2b is 2^128 - (2^(130-b) - 2^(130-2b) - 2^b) < 2^128 for 44 <= b <= 63, and with e capped
// at 32 (b < 48) stays below 2^(33+2b) < 2^128.  Every accumulator here takes ONE product a ciphertext (component
// i of the learner's ciphertext times the plaintext), where dot's c1 takes two: a run may hold all P
// ciphertexts, 256 on a 60-bit tower where dot_fold_interval gives 128, 2^32 from 48 bits down.
__device__ __forceinline__ uint64_t dotp_fold_interval(uint64_t q) {
  const int b = 64 - __builtin_clzll(q);
  const int e = max(min(128 - 2 * b, 32), 0);  // (b <= 60 in every chain the library builds)
  return 1ull << e;
}

// ciphertexts loaded before any is used, 2 NC + NR 16-byte loads each: as many as keep up to 12 loads in
// flight a thread, but two for the 1 x 2 tile, whose third costs it half its waves (182 registers against
// 108: DESIGN.md §2.16's table, which these are chosen from: loads a thread x waves a SIMD is the figure kept up)
template <int NC, int NR>
constexpr int dotp_unroll() {
  return NC == 1 && NR == 2 ? 2 : std::max(1, 12 / (2 * NC + NR));
}

// Grid (512-coefficient block, tower, tile x slice) over the ntr-wide grid of NC x NR tiles whose first
// learner is c0 and first plaintext r0; one thread = 2 adjacent coefficients (dot_partial_kernel's
// arrangement: the tower is block-uniform, so its constants sit in SGPRs; 16-byte non-temporal loads; 128-bit
// accumulators with no reduction inside a run of dotp_fold_interval ciphertexts).  A narrower instance runs
// the same sums on fewer pairs, so ragged edges give the same bits.  dst [S][C R][2][Ll][N]: the partials, or
// (S = 1) out itself.  Nothing here needs TowerConst::red_ok: 30-bit chains run the same code.
template <int NC, int NR>
__global__ __launch_bounds__(256) void dotp_partial_kernel(const DotpArgs g, const uint64_t* __restrict__ pts,
                                                           uint32_t c0, uint32_t r0, uint32_t ntr, uint32_t CR,
                                                           uint32_t R, uint64_t K, uint32_t S, uint32_t Ll,
                                                           uint32_t logN, const TowerConst* __restrict__ tq,
                                                           uint64_t* __restrict__ dst) {
  constexpr int U = dotp_unroll<NC, NR>();
  const uint32_t t = blockIdx.y, s = blockIdx.z % S, tile = blockIdx.z / S;
  const uint32_t cb = c0 + (tile / ntr) * NC, rb = r0 + (tile % ntr) * NR;
  const TowerConst c = tq[t];
  const uint64_t k0 = (uint64_t)s * K / S, k1 = (uint64_t)(s + 1) * K / S;  // balanced: no empty slice (S <= K)
  const uint64_t G = dotp_fold_interval(c.q);
  const uint64_t poly = (uint64_t)Ll << logN, ctw = 2 * poly;
  const uint64_t off = ((uint64_t)t << logN) + (uint64_t)blockIdx.x * 512 + 2u * threadIdx.x;
  const uint64_t* A[NC];
  const uint64_t* P[NR];
#pragma unroll
  for (int l = 0; l < NC; ++l) A[l] = g.u[cb + l] + off;
#pragma unroll
  for (int j = 0; j < NR; ++j) P[j] = pts + (uint64_t)(rb + j) * K * poly + off;
  du128 acc[NC][NR][2][2];  // [learner][plaintext][component][coefficient]
#pragma unroll
  for (int l = 0; l < NC; ++l)
#pragma unroll
    for (int j = 0; j < NR; ++j)
#pragma unroll
      for (int i = 0; i < 2; ++i) acc[l][j][i][0] = acc[l][j][i][1] = 0;
  const auto step = [&](uint64_t k, auto n) {
    constexpr int V = decltype(n)::value;
    ulonglong2 a[V][NC][2], p[V][NR];
#pragma unroll
    for (int u = 0; u < V; ++u) {
#pragma unroll
      for (int l = 0; l < NC; ++l) {
        a[u][l][0] = ld_pair(A[l] + (k + u) * ctw);
        a[u][l][1] = ld_pair(A[l] + (k + u) * ctw + poly);
      }
#pragma unroll
      for (int j = 0; j < NR; ++j) p[u][j] = ld_pair(P[j] + (k + u) * poly);
    }
#pragma unroll
    for (int u = 0; u < V; ++u)
#pragma unroll
      for (int l = 0; l < NC; ++l)
#pragma unroll
        for (int j = 0; j < NR; ++j)
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            acc[l][j][i][0] += (du128)a[u][l][i].x * p[u][j].x;
            acc[l][j][i][1] += (du128)a[u][l][i].y * p[u][j].y;
          }
  };
  uint64_t k = k0;
  while (k < k1) {
    const uint64_t ke = min(k1, k + G);
    for (; k + U <= ke; k += U) step(k, std::integral_constant<int, U>());
    for (; k < ke; ++k) step(k, std::integral_constant<int, 1>());
#pragma unroll
    for (int l = 0; l < NC; ++l)
#pragma unroll
      for (int j = 0; j < NR; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          acc[l][j][i][0] = dot_red128(acc[l][j][i][0], c);
          acc[l][j][i][1] = dot_red128(acc[l][j][i][1], c);
        }
  }
  uint64_t* __restrict__ o = dst + (uint64_t)s * CR * ctw + off;
#pragma unroll
  for (int l = 0; l < NC; ++l)
#pragma unroll
    for (int j = 0; j < NR; ++j)
#pragma unroll
      for (int i = 0; i < 2; ++i)
        *reinterpret_cast<ulonglong2*>(o + ((uint64_t)(cb + l) * R + rb + j) * ctw + i * poly) =
            make_ulonglong2((uint64_t)acc[l][j][i][0], (uint64_t)acc[l][j][i][1]);
}

// One thread = one 16-byte residue pair of a polynomial row (rows = C R 2 Ll, tower = row % Ll): the S <= 16
// canonical partials of each residue summed as plain uint64 (16 q < 2^64 for q < 2^60: dot_reduce_block's
// argument) and folded by one red64.  words: from slice to slice of part.
__global__ __launch_bounds__(256) void dotp_reduce_kernel(const uint64_t* __restrict__ part, uint64_t words, uint32_t S,
                                                          uint32_t Ll, uint32_t logN,
                                                          const TowerConst* __restrict__ tq,
                                                          uint64_t* __restrict__ out) {
  const uint32_t bpr = 1u << (logN - 9);  // blocks per row: 256 threads x 2 residues
  const uint64_t row = blockIdx.x / bpr;
  const TowerConst& c = tq[row % Ll];
  const uint64_t i = (row << (logN - 1)) + (uint64_t)(blockIdx.x % bpr) * 256 + threadIdx.x;
  ulonglong2 r = make_ulonglong2(0, 0);
  for (uint32_t s = 0; s < S; ++s) {
    const ulonglong2 v = reinterpret_cast<const ulonglong2*>(part + s * words)[i];
    r.x += v.x;
    r.y += v.y;
  }
  reinterpret_cast<ulonglong2*>(out)[i] = make_ulonglong2(red64(r.x, c.q, c.one_shoup), red64(r.y, c.q, c.one_shoup));
}

// The tiling: 2 x 2 tiles with the ragged edges of an odd C or R narrower; one plaintext batch (R = 1, a score
// against one known vector) takes the learners four, then two, then one at a time.
uint64_t dotp_tiles(uint64_t C, uint64_t R) {
  if (R == 1) return C / 4 + ((C & 2) >> 1) + (C & 1);
  return ((C + 1) / 2) * ((R + 1) / 2);
}

// Slices of the K ciphertexts: gram's rule -- ceil(K / slice_cts), at most kDotMaxSlices, but no more than bring
// the call's workgroups (tiles x towers x 512-coefficient blocks) to kGramFillGroups -- lowered until the
// partials [S][C R][2][Ll][N] fit budget_bytes; one slice has none.
uint32_t dotp_slices(uint64_t C, uint64_t R, uint64_t K, uint32_t Ll, uint32_t logN, uint64_t slice_cts,
                     uint64_t budget_bytes) {
  const uint64_t groups = dotp_tiles(C, R) * Ll << (logN > 9 ? logN - 9 : 0);
  const uint64_t fill = (kGramFillGroups + groups - 1) / groups;
  const uint64_t per = std::max<uint64_t>(1, slice_cts);
  uint32_t S = (uint32_t)std::min<uint64_t>({(uint64_t)kDotMaxSlices, fill, K / per + (K % per ? 1 : 0)});
  while (S > 1 && dotp_scratch_bytes(C, R, Ll, logN, S) > budget_bytes) --S;
  return S;
}

size_t dotp_scratch_bytes(uint64_t C, uint64_t R, uint32_t Ll, uint32_t logN, uint32_t S) {
  return S > 1 ? ((size_t)S * C * R * 2 * Ll << logN) * 8 : 0;
}

void launch_dotp(const uint64_t* const* u, uint32_t C, const uint64_t* pts, uint32_t R, uint64_t K, uint32_t S,
                 uint32_t Ll, uint32_t logN, const TowerConst* tq, uint64_t* out, void* scratch, hipStream_t s) {
  if (logN < 9) throw Error{SHELFI_ERR_ARG, "EvalInnerProduct(ct, pt): unsupported ring dimension"};
  if (C < 1 || C > (uint32_t)kDotpMaxBatches || R < 1 || R > (uint32_t)kDotpMaxBatches || !K)
    throw Error{SHELFI_ERR_ARG, "EvalInnerProduct(ct, pt): bad shape"};
  if (S < 1 || S > (uint32_t)kDotMaxSlices || S > K || (S > 1 && !scratch))
    throw Error{SHELFI_ERR_ARG, "EvalInnerProduct(ct, pt): bad slice count"};
  DotpArgs g{};
  for (uint32_t i = 0; i < C; ++i) g.u[i] = u[i];
  uint64_t* dst = S > 1 ? static_cast<uint64_t*>(scratch) : out;
  // the ntc x ntr grid of one tile shape whose first learner is c0 and first plaintext r0
  const auto tiles = [&](auto kernel, uint32_t c0, uint32_t ntc, uint32_t r0, uint32_t ntr) {
    if (!ntc || !ntr) return;
    hipLaunchKernelGGL(kernel, dim3(1u << (logN - 9), Ll, ntc * ntr * S), dim3(256), 0, s, g, pts, c0, r0, ntr, C * R, R, K,
                       S, Ll, logN, tq, dst);
    SHELFI_HIP(hipGetLastError());
  };
  if (R == 1) {
    tiles(dotp_partial_kernel<4, 1>, 0, C / 4, 0, 1);
    tiles(dotp_partial_kernel<2, 1>, C & ~3u, (C & 2) >> 1, 0, 1);
    tiles(dotp_partial_kernel<1, 1>, C & ~1u, C & 1, 0, 1);
  } else {
    tiles(dotp_partial_kernel<2, 2>, 0, C / 2, 0, R / 2);
    tiles(dotp_partial_kernel<2, 1>, 0, C / 2, R & ~1u, R & 1);
    tiles(dotp_partial_kernel<1, 2>, C & ~1u, C & 1, 0, R / 2);
    tiles(dotp_partial_kernel<1, 1>, C & ~1u, C & 1, R & ~1u, R & 1);
  }
  if (S == 1) return;
  const uint64_t rows = (uint64_t)C * R * 2 * Ll;
  hipLaunchKernelGGL(dotp_reduce_kernel, dim3((uint32_t)(rows << (logN - 9))), dim3(256), 0, s, dst, rows << logN, S, Ll,
                     logN, tq, out);
  SHELFI_HIP(hipGetLastError());
}

}  // namespace shelfi
