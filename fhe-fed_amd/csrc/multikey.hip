// multikey.hip — the multiparty evaluation-key protocols of threshold CKKS on gfx950 (the
// reference's code/mkhe/mkhe.cpp:271-317), on this project's HYBRID keys.
//
// P parties hold additive shares s_i of one secret s = sum s_i.  Keys are in the evaluation key's
// layout [2][dnum][L + kP][N] (b-vector, a-vector), EVALUATION, towers of Q then of P:
//   round 1  (KeySwitchGen(sk, sk) :271 for the lead, MultiKeySwitchGen :296 / MultiEvalSumKeyGen
//            :284 for the others)
//              b_{i,j} = NTT(e_{i,j}) - a_j s_i + [t in digit j] (P mod q_t) s'_i
//            s'_i = s_i (the EvalMult share) or sigma_g(s_i) (a rotation share); a_j is drawn by the
//            lead party and copied, bit for bit, by everybody else.
//   add      (MultiAddEvalKeys :298, MultiAddEvalSumKeys :288) b-vectors summed, a-vectors equal:
//            b = sum e - a s + [digit] P s' -- for a rotation index already a rotation key under s.
//   round 2  (MultiMultEvalKey :307, :311) b'_{i,j} = b_j s_i + NTT(E2_{i,j}), a'_{i,j} = a_j s_i +
//            NTT(E1_{i,j}); MultiAddEvalMultKeys (:314) sums both vectors: an EvalMult key under s.
//
// Streams: the context's ChaCha20 key; round 1 nonce (7 << 56) | (g << 24) | (j << 16) | (1 + t) for
// a_{j,t} (evk_sample_kernel's layout; t-field 0 for e_j; g = 1 for the EvalMult share, which no
// rotation uses), round 2 nonce (8 << 56) | (v << 24) | (j << 16), words [0, N) the error of the
// b-vector (v = 0) or the a-vector (v = 1).
//
// Every kernel is elementwise over the key: 256-thread workgroups, TowerConst per tower.
#include <hip/hip_runtime.h>

#include "dev_common.h"
#include "shelfi_internal.h"

namespace shelfi {

// An error polynomial alone, e [T0][N] (COEFFICIENT, the same small integers mod every tower):
// evk_sample_kernel without the two ChaCha20 blocks per tower of its uniform draw.  One thread per
// 8 coefficients (one ChaCha20 block).
__global__ __launch_bounds__(256) void mk_error_sample_kernel(uint32_t logN, uint32_t T0,
                                                              const TowerConst* __restrict__ te,
                                                              const uint64_t* __restrict__ cdt, int T, Key8 key,
                                                              uint64_t nonce, uint64_t* __restrict__ e_out) {
  const uint32_t N = 1u << logN;
  const uint32_t gid = blockIdx.x * 256 + threadIdx.x;
  if (gid >= (N >> 3)) return;
  const uint32_t j0 = gid * 8;
  uint64_t re[8];
  chacha20_block(key, j0 >> 3, nonce, re);
  int64_t ev[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) ev[u] = gauss_sample(re[u], cdt, T);
  for (uint32_t t = 0; t < T0; ++t) {
    const TowerConst c = te[t];
    ulonglong2* o = reinterpret_cast<ulonglong2*>(e_out + (uint64_t)t * N + j0);
#pragma unroll
    for (int u = 0; u < 8; u += 2)
      o[u >> 1] = make_ulonglong2(mod_signed_dev(ev[u], c), mod_signed_dev(ev[u + 1], c));
  }
}

// A share's digit j: b = e - a s + [t in digit j] (P mod q_t) s' with s' = s (galois = 1) or
// sigma_g(s) gathered through the automorphism's index map; a from `a_src` [T0][N] -- the fresh draw,
// or digit j of the previous key's a-vector, whose words (and those of its b-vector, prev_b, when
// given) are range-checked.  out[0][j] = b, out[1][j] = a.
__global__ __launch_bounds__(256) void mk_share_combine_kernel(const uint64_t* __restrict__ e_eval,
                                                               const uint64_t* __restrict__ a_src,
                                                               const uint64_t* __restrict__ prev_b,
                                                               const uint64_t* __restrict__ sk,
                                                               const uint64_t* __restrict__ sp,
                                                               const TowerConst* __restrict__ te, EvkGenConst g,
                                                               uint32_t galois, uint32_t j,
                                                               uint32_t* __restrict__ flag,
                                                               uint64_t* __restrict__ out) {
  const uint32_t N = 1u << g.logN, T0 = g.L + g.kP;
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (uint64_t)T0 * N) return;
  const uint32_t t = (uint32_t)(e >> g.logN);
  const TowerConst c = te[t];
  const uint64_t st = t < g.L ? sk[e] : sp[e - (uint64_t)g.L * N];
  const uint64_t a = a_src[e];
  if (a >= c.q || (prev_b && prev_b[e] >= c.q)) atomicOr(flag, kMkBadResidue);
  uint64_t b = submod(e_eval[e], mulmod_generic(a, st, c), c.q);
  if (t < g.L && t >= j * g.alpha && t < (j + 1) * g.alpha) {
    // (only towers of Q carry the P s' term: sp, s over P, needs no gather)
    const uint64_t sn =
        galois == 1 ? st : sk[((uint64_t)t << g.logN) + galois_src((uint32_t)(e & (N - 1)), galois, g.logN)];
    b = addmod(b, mulmod_generic(g.pmod[t], sn, c), c.q);
  }
  const uint64_t TN = (uint64_t)T0 * N;
  out[(uint64_t)j * TN + e] = b;
  out[((uint64_t)g.dnum + j) * TN + e] = a;
}

// Round 2 of digit j, both vectors in one launch: out[v][j] = joint[v][j] s + E_v, E [2][T0][N] in
// EVALUATION (E2 for the b-vector, then E1 for the a-vector); the joint key's words are range-checked.
__global__ __launch_bounds__(256) void mk_round2_kernel(const uint64_t* __restrict__ joint,
                                                        const uint64_t* __restrict__ E,
                                                        const uint64_t* __restrict__ sk,
                                                        const uint64_t* __restrict__ sp,
                                                        const TowerConst* __restrict__ te, EvkGenConst g,
                                                        uint32_t j, uint32_t* __restrict__ flag,
                                                        uint64_t* __restrict__ out) {
  const uint32_t N = 1u << g.logN, T0 = g.L + g.kP;
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (uint64_t)T0 * N) return;
  const uint32_t t = (uint32_t)(e >> g.logN);
  const TowerConst c = te[t];
  const uint64_t st = t < g.L ? sk[e] : sp[e - (uint64_t)g.L * N];
  const uint64_t TN = (uint64_t)T0 * N;
#pragma unroll
  for (uint32_t v = 0; v < 2; ++v) {
    const uint64_t at = ((uint64_t)v * g.dnum + j) * TN + e;
    const uint64_t x = joint[at];
    if (x >= c.q) atomicOr(flag, kMkBadResidue);
    out[at] = addmod(mulmod_generic(x, st, c), E[(uint64_t)v * TN + e], c.q);
  }
}

// The sum of k.n <= 16 keys, 16 bytes per thread: uint64 sums of canonical residues (below 2^60, so
// 16 of them cannot wrap) folded once.  The b-vector always; the a-vector too (sum_a), or else compared
// word for word with the first key's, which is kept.  Every word is range-checked.
__global__ __launch_bounds__(256) void mk_key_add_kernel(MkKeys k, uint64_t half_words, uint32_t T0,
                                                         uint32_t logN, const TowerConst* __restrict__ te,
                                                         uint32_t sum_a, uint32_t* __restrict__ flag,
                                                         uint64_t* __restrict__ out) {
  const uint64_t w = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 2;
  if (w >= 2 * half_words) return;
  const bool a_half = w >= half_words;
  const uint32_t t = (uint32_t)(((a_half ? w - half_words : w) >> logN) % T0);  // N >= 2: one tower per pair
  const TowerConst c = te[t];
  const ulonglong2 first = *reinterpret_cast<const ulonglong2*>(k.k[0] + w);
  ulonglong2 acc = first;
  uint32_t bad = (first.x >= c.q || first.y >= c.q) ? kMkBadResidue : 0;
  for (uint32_t i = 1; i < k.n; ++i) {
    const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(k.k[i] + w);
    if (v.x >= c.q || v.y >= c.q) bad |= kMkBadResidue;
    if (a_half && !sum_a) {
      if (v.x != first.x || v.y != first.y) bad |= kMkADiffers;
    } else {
      acc.x += v.x;
      acc.y += v.y;
    }
  }
  if (bad) atomicOr(flag, bad);
  *reinterpret_cast<ulonglong2*>(out + w) =
      make_ulonglong2(red64(acc.x, c.q, c.one_shoup), red64(acc.y, c.q, c.one_shoup));
}

static dim3 mk_grid(uint64_t threads) {
  const uint64_t b = (threads + 255) / 256;
  if (b > 0x7FFFFFFFull) throw Error{SHELFI_ERR_ARG, "multiparty key: ring too large"};
  return dim3((uint32_t)b);
}

static Key8 mk_key8(const uint32_t key[8]) {
  Key8 k8;
  for (int i = 0; i < 8; ++i) k8.k[i] = key[i];
  return k8;
}

void launch_mk_share(const EvkGenConst& g, const DeviceTables& dtq, const DeviceTables& dte, const uint64_t* cdt,
                     int cdt_len, const uint32_t key[8], const uint64_t* sk, uint32_t galois,
                     const uint64_t* prev, uint64_t* out, void* scratch, uint32_t* flag, hipStream_t s) {
  const uint32_t N = 1u << g.logN, T0 = g.L + g.kP;
  const uint64_t tn = (uint64_t)T0 * N;
  const uint64_t nonce_base = (7ull << 56) | ((uint64_t)galois << 24);
  uint64_t* eb = reinterpret_cast<uint64_t*>(scratch);
  uint64_t* ab = eb + tn;
  uint64_t* sp = ab + tn;
  uint64_t* s0 = sp + (uint64_t)g.kP * N;
  const Key8 k8 = mk_key8(key);
  launch_evk_s_ext(g, dtq, dte, sk, sp, s0, s);
  for (uint32_t j = 0; j < g.dnum; ++j) {
    if (prev) {
      hipLaunchKernelGGL(mk_error_sample_kernel, mk_grid(N / 8), dim3(256), 0, s, g.logN, T0, dte.tc, cdt, cdt_len,
                         k8, nonce_base | ((uint64_t)j << 16), eb);
      SHELFI_HIP(hipGetLastError());
    } else {
      launch_evk_sample(g, dte, cdt, cdt_len, key, nonce_base, j, eb, ab, s);
    }
    launch_ntt(eb, T0, T0, g.logN, false, dte, s);
    hipLaunchKernelGGL(mk_share_combine_kernel, mk_grid(tn), dim3(256), 0, s, eb,
                       prev ? prev + ((uint64_t)g.dnum + j) * tn : ab, prev ? prev + (uint64_t)j * tn : nullptr, sk,
                       sp, dte.tc, g, galois, j, flag, out);
    SHELFI_HIP(hipGetLastError());
  }
}

void launch_mk_round2(const EvkGenConst& g, const DeviceTables& dtq, const DeviceTables& dte, const uint64_t* cdt,
                      int cdt_len, const uint32_t key[8], const uint64_t* sk, const uint64_t* joint,
                      uint64_t* out, void* scratch, uint32_t* flag, hipStream_t s) {
  const uint32_t N = 1u << g.logN, T0 = g.L + g.kP;
  const uint64_t tn = (uint64_t)T0 * N;
  uint64_t* eb = reinterpret_cast<uint64_t*>(scratch);  // E2 | E1, contiguous: one NTT batch
  uint64_t* sp = eb + 2 * tn;
  uint64_t* s0 = sp + (uint64_t)g.kP * N;
  const Key8 k8 = mk_key8(key);
  launch_evk_s_ext(g, dtq, dte, sk, sp, s0, s);
  for (uint32_t j = 0; j < g.dnum; ++j) {
    for (uint64_t v = 0; v < 2; ++v) {
      hipLaunchKernelGGL(mk_error_sample_kernel, mk_grid(N / 8), dim3(256), 0, s, g.logN, T0, dte.tc, cdt, cdt_len,
                         k8, (8ull << 56) | (v << 24) | ((uint64_t)j << 16), eb + v * tn);
      SHELFI_HIP(hipGetLastError());
    }
    launch_ntt(eb, 2ull * T0, T0, g.logN, false, dte, s);
    hipLaunchKernelGGL(mk_round2_kernel, mk_grid(tn), dim3(256), 0, s, joint, eb, sk, sp, dte.tc, g, j, flag, out);
    SHELFI_HIP(hipGetLastError());
  }
}

void launch_mk_key_add(const MkKeys& k, const EvkGenConst& g, const TowerConst* te, bool sum_a, uint32_t* flag,
                       uint64_t* out, hipStream_t s) {
  const uint32_t T0 = g.L + g.kP;
  const uint64_t half = ((uint64_t)g.dnum * T0) << g.logN;
  hipLaunchKernelGGL(mk_key_add_kernel, mk_grid(half), dim3(256), 0, s, k, half, T0, g.logN, te, sum_a ? 1u : 0u,
                     flag, out);
  SHELFI_HIP(hipGetLastError());
}

}  // namespace shelfi
