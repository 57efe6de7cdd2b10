// dev_api.cpp — the device API (shelfi_dev_*: device buffers in, device buffers out, the caller's
// stream) and the packed resident arena it aggregates from.
#include <cmath>
#include <cstring>
#include <mutex>

#include "api_internal.h"
#include "api_util.h"

using namespace shelfi;

namespace shelfi {

// Weight limbs [C][L][2] of wavg_packed in a device buffer: a ring of slots, the
// last one reused while the weights repeat (every step of a round), a slot rewritten
// only after the kernels that read it have completed.
static int arena_weight_slot(shelfi_ctx* ctx, const float* w, size_t C, hipStream_t s) {
  const Params& p = ctx->p;
  std::vector<uint32_t> wl(C * p.L * 2);
  for (size_t c = 0; c < C; ++c) weight_limbs(w[c], p, &wl[c * p.L * 2]);
  const int last = ctx->wl_last_slot;
  if (last >= 0 && ctx->wl_host[last] == wl) return last;
  const int i = ctx->wl_next;
  ctx->wl_next = (i + 1) % shelfi_ctx::kWeightRing;
  if (ctx->wl_done[i]) SHELFI_HIP(hipEventSynchronize(ctx->wl_done[i]));
  else SHELFI_HIP(hipEventCreateWithFlags(&ctx->wl_done[i], hipEventDisableTiming));
  const size_t bytes = wl.size() * sizeof(uint32_t);
  if (ctx->wl_cap[i] < bytes) {
    if (ctx->wl_dev[i]) (void)hipFree(ctx->wl_dev[i]);
    ctx->wl_dev[i] = nullptr;
    ctx->wl_cap[i] = 0;
    SHELFI_HIP(hipMalloc(&ctx->wl_dev[i], bytes));
    ctx->wl_cap[i] = bytes;
  }
  ctx->wl_host[i] = std::move(wl);  // stays alive until the slot is reused
  SHELFI_HIP(hipMemcpyAsync(ctx->wl_dev[i], ctx->wl_host[i].data(), bytes, hipMemcpyHostToDevice, s));
  ctx->wl_last_slot = i;
  return i;
}

// The refusal bookkeeping of one put into slot `learner` of the arena [arena, arena + words) of C
// learners (ctx lock held): the slot's earlier entry is superseded, and so is every entry that
// overlaps this arena but names another base, span or learner count (that arena was freed and
// this memory reused); a refused put records the slot.
static void arena_mark(shelfi_ctx* ctx, const uint64_t* arena, size_t words, size_t C, size_t learner,
                       bool refused) {
  auto& R = ctx->arena_refused;
  for (size_t i = 0; i < R.size();) {
    const auto& r = R[i];
    const bool same_arena = r.arena == arena && r.words == words && r.C == C;
    const bool overlaps = arena < r.arena + r.words && r.arena < arena + words;
    if ((same_arena && r.learner == learner) || (overlaps && !same_arena)) R.erase(R.begin() + (long)i);
    else ++i;
  }
  if (refused) R.push_back({arena, words, C, learner});
}

// Placement of a learner's batch into its packed slices (arena_pack_kernel: the canonical-residue
// check of every residue rides along, ~0.3 ms of HBM per 1.4 GiB against ~30 ms of PCIe for the
// upload), then the slot's refusal mark is set or cleared.  `rows_of(k0, kn, dst)` makes
// ciphertexts [k0, k0 + kn) available as contiguous [kn][2][L][N] device residues and returns
// them (a device batch: the caller's pointer; host data: staged through `dst`, the context's
// scratch, `chunk` ciphertexts at a time).  Synchronises `s`.  Called under the ctx lock.
template <class RowsOf>
static void arena_place(shelfi_ctx* ctx, size_t K, size_t learner, size_t C, uint64_t* arena_dev, hipStream_t s,
                        size_t chunk, bool staged, RowsOf rows_of) {
  const Params& p = ctx->p;
  const ArenaPack ap = arena_pack(p);
  uint32_t* bad = ctx->dev_flag + 4;
  SHELFI_HIP(hipMemsetAsync(bad, 0, 4, s));
  const uint64_t ct_rows = 2ull * p.L * (p.N / kArenaChunk);
  uint64_t* dst = nullptr;
  if (staged)
    dst = (uint64_t*)ensure(ctx->scratch, ctx->scratch_bytes, std::min(chunk, K) * 2ull * p.L * p.N * 8);
  for (size_t k0 = 0; k0 < K; k0 += chunk) {
    const size_t kn = std::min(chunk, K - k0);
    const uint64_t* src = rows_of(k0, kn, dst);
    launch_arena_pack(src, k0 * ct_rows, kn * ct_rows, (uint32_t)C, (uint32_t)learner, p.L, p.logN, ap,
                      ctx->dt.tc, arena_dev, bad, s);
  }
  uint32_t flag = 0;
  SHELFI_HIP(hipMemcpyAsync(&flag, bad, 4, hipMemcpyDeviceToHost, s));
  SHELFI_HIP(hipStreamSynchronize(s));
  arena_mark(ctx, arena_dev, (size_t)arena_ct_words(p, C) * K, C, learner, flag != 0);
  if (flag)
    throw Error{SHELFI_ERR_FORMAT,
                "learner " + std::to_string(learner) +
                    ": ciphertext residue >= its tower modulus (malformed upload; the arena slot is "
                    "marked refused until a valid upload replaces it)"};
}
// How host uploads reach the device: a contiguous run (a library blob's payload, a host batch) as one
// hipMemcpyAsync from the caller's pageable memory (54 GB/s for a 1.5 GB upload), the 2 L tower runs
// of 256 KiB per ciphertext of a PALISADE archive through the bytes API's pinned staging ring (49 vs
// 18.5 GB/s as separate copies; probes/r03_arena_put.txt).  SHELFI_ARENA_STAGER=0|1 forces one (A/B
// probe switch).
static bool arena_use_stager(size_t pieces, size_t bytes) {
  if (switches().arena_stager >= 0) return switches().arena_stager == 1;
  return pieces > 1 && bytes / pieces < (4u << 20);
}
// Host uploads are staged through the scratch in pieces of about 64 MiB.
static size_t arena_stage_cts(const Params& p) {
  return std::max<size_t>(1, (64ull << 20) / (2ull * p.L * p.N * 8));
}

// Packed widths of the resident arena: U_t = bitlength(q_t) when that is 1 mod 4 (a
// 4-multiple field + a flag plane for the top bit), else 4 ceil(bitlength(q_t) / 4); at least 32.
ArenaPack arena_pack(const Params& p) {
  ArenaPack ap;
  std::memset(&ap, 0, sizeof(ap));
  for (uint32_t t = 0; t < p.L; ++t) {
    const uint32_t bits = 64 - (uint32_t)__builtin_clzll(p.q[t]);
    const uint32_t U = bits <= 32 ? 32u : (bits % 4 == 1 ? bits : (bits + 3) & ~3u);
    if (U > 60) throw Error{SHELFI_ERR_ARG, "arena: modulus above 2^60"};
    ap.w[t] = U;
    ap.pre[t] = ap.sum;
    ap.sum += U;
  }
  return ap;
}
// uint64 words per ciphertext of a C-learner arena: 2 N sum_t U_t / 64 per learner
uint64_t arena_ct_words(const Params& p, uint64_t C) {
  return C * 2ull * (p.N / kArenaChunk) * 8ull * arena_pack(p).sum;
}

// An aggregation over arena words [a, a + words) must not read a refused slot (ctx lock held).
void arena_require_valid_locked(const shelfi_ctx* ctx, const uint64_t* a, size_t words) {
  for (const auto& r : ctx->arena_refused)
    if (a < r.arena + r.words && r.arena < a + words)
      throw Error{SHELFI_ERR_STATE, "the arena holds a refused upload for learner " +
                                        std::to_string(r.learner) + "; put a valid batch first"};
}

// The arena aggregation itself (ctx lock held, weights checked): one wavg_packed pass over any
// number of learners (groups of 16 folded into a running sum), weight limbs from the device ring.
void wavg_arena_enqueue(shelfi_ctx* ctx, const uint64_t* arena_dev, const float* w, size_t C, size_t K,
                        uint64_t* out_dev, hipStream_t s) {
  const Params& p = ctx->p;
  const int slot = arena_weight_slot(ctx, w, C, s);
  launch_wavg_packed(arena_dev, ctx->wl_dev[slot], (uint32_t)C, (uint64_t)K * 2 * p.L, p.L, p.logN, arena_pack(p),
                     ctx->dt.tc, out_dev, s);
  SHELFI_HIP(hipEventRecord(ctx->wl_done[slot], s));
}

// The same aggregation with its result written in the packed C = 1 layout (the packed share
// exchange's send buffer): out_packed receives K ciphertexts, arena_ct_words(p, 1) words each.
void wavg_arena_enqueue_packed(shelfi_ctx* ctx, const uint64_t* arena_dev, const float* w, size_t C, size_t K,
                               uint64_t* out_packed, hipStream_t s) {
  const Params& p = ctx->p;
  const int slot = arena_weight_slot(ctx, w, C, s);
  launch_wavg_packed_ex(reinterpret_cast<const uint32_t*>(arena_dev), ctx->wl_dev[slot], (uint32_t)C, (uint32_t)C,
                        0, (uint64_t)K * 2 * p.L, p.L, p.logN, arena_pack(p), ctx->dt.tc, nullptr,
                        reinterpret_cast<uint32_t*>(out_packed), s);
  SHELFI_HIP(hipEventRecord(ctx->wl_done[slot], s));
}

// sum_g x_g mod q_t over G packed C = 1 batches of K ciphertexts stacked `stride` uint64 words apart
// (the packed share exchange's receive buffer) -> uint64 [K][2][L][N] canonical: wavg_packed with
// unit weight limbs (w0 = 1, w1 = 0), so the fold is the mod-q reduction.
void sum_packed_enqueue(shelfi_ctx* ctx, const uint64_t* stacked, size_t G, size_t K, size_t stride,
                        uint64_t* out, hipStream_t s) {
  const Params& p = ctx->p;
  if (!G || G > (size_t)kMaxCommRanks) throw Error{SHELFI_ERR_ARG, "sum_packed: 1..16 batches"};
  if (stride < (size_t)arena_ct_words(p, 1) * K) throw Error{SHELFI_ERR_ARG, "sum_packed: stride below the batch"};
  if (!ctx->unit_wl) {
    std::vector<uint32_t> one((size_t)kMaxCommRanks * kMaxTowers * 2, 0);
    for (size_t i = 0; i < one.size(); i += 2) one[i] = 1;
    SHELFI_HIP(hipMalloc(&ctx->unit_wl, one.size() * sizeof(uint32_t)));
    SHELFI_HIP(hipMemcpy(ctx->unit_wl, one.data(), one.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  if (!K) return;
  launch_wavg_packed_ex(reinterpret_cast<const uint32_t*>(stacked), ctx->unit_wl, (uint32_t)G, 1, 2ull * stride,
                        (uint64_t)K * 2 * p.L, p.L, p.logN, arena_pack(p), ctx->dt.tc, out, nullptr, s);
}

// Ciphertexts per launch chain of the device-resident encrypt/decrypt: as many as a
// 4 GiB scratch holds (1149 at N = 2^15, L = 4: one chain for a ResNet-18 learner),
// split into equal chunks, so no launch runs a short tail chunk.
// SHELFI_DEV_CHUNK_MIB overrides the budget (A/B probe switch).
static uint64_t dev_chunk(uint64_t K, size_t scratch_per_ct) {
  const uint64_t mib = switches().dev_chunk_mib;
  const uint64_t cap = std::max<uint64_t>(1, (mib << 20) / scratch_per_ct);
  const uint64_t n = (K + cap - 1) / cap;
  return n ? (K + n - 1) / n : 1;
}

// decrypt K ciphertexts of `towers` RNS towers (the context's L, or fewer after ModReduce)
// (sum_in: residues are uint64 sums of <= 16 canonical residues, folded on load; fuse: threshold
// fusion -- no ciphertexts and no key, the first pass sums fuse->P partial decryptions [K][towers][N]).
// The caller holds ctx->mu, has selected the device and checked the keys.
void dev_decrypt_locked(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, uint32_t towers, double scale, size_t n,
                        double* out_dev, hipStream_t s, bool sum_in, const FuseIn* fuse) {
  if (towers < 1 || towers > ctx->p.L) throw Error{SHELFI_ERR_ARG, "tower count out of range for this context"};
  if (n > (uint64_t)K * ctx->p.batch) throw Error{SHELFI_ERR_ARG, "n exceeds the slots in K ciphertexts"};
  const uint64_t Kn = (n + ctx->p.batch - 1) / ctx->p.batch;
  if (!Kn) return;
  const size_t ct_words = 2ull * towers * ctx->p.N, part_words = (size_t)towers * ctx->p.N;
  const GenFlag fl = next_gen_flag(ctx);
  DecodeNoise dn = decode_noise_begin(ctx, Kn, fl);
  const uint64_t g0 = dn.g0;
  // one pass over the call: the decode's tower prefix with the fast CRT, or (exact) every tower
  // through crt_exact_kernel
  const auto run = [&](bool exact) {
    const DecodePass pass = decode_pass(ctx, towers, exact);
    const Params& p = pass.p;
    const DeviceTables& dt = pass.dt;
    const uint64_t kc_max = dev_chunk(Kn, decrypt_scratch_bytes(p, 1));
    void* scratch = ensure(ctx->scratch, ctx->scratch_bytes, decrypt_scratch_bytes(p, kc_max));
    dn.reset = 1;
    for (uint64_t k0 = 0; k0 < Kn; k0 += kc_max) {
      const uint64_t kc = std::min(kc_max, Kn - k0);
      const uint64_t o0 = k0 * p.batch, on = std::min<uint64_t>(n - o0, kc * p.batch);
      dn.g0 = g0 + k0;
      if (fuse) {
        FuseIn fz = *fuse;
        for (uint32_t i = 0; i < fz.P; ++i) fz.part[i] += k0 * part_words;
        launch_decrypt(p, dt, ctx->dk, nullptr, kc, scale, on, out_dev + o0, scratch, s, &dn, false, towers, fl,
                       exact, &fz);
      } else {
        launch_decrypt(p, dt, ctx->dk, ct_dev + k0 * ct_words, kc, scale, on, out_dev + o0, scratch, s, &dn,
                       sum_in, towers, fl, exact);
      }
      dn.reset = 0;  // the flags are reset by the first chunk's flooding only
    }
    decode_noise_readback(ctx, dn);
  };
  // the wait after the last pass: scratch is reused by the next call
  decrypt_passes(ctx, fl, dn, run, [&] { SHELFI_HIP(hipStreamSynchronize(s)); });
}

static int dev_decrypt(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, uint32_t towers, double scale,
                       size_t n, double* out_dev, void* stream, bool sum_in = false) {
  if (!ctx || (n && (!ct_dev || !out_dev))) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    require_keys(ctx);
    DeviceGuard g(ctx->device);
    dev_decrypt_locked(ctx, ct_dev, K, towers, scale, n, out_dev, (hipStream_t)stream, sum_in, nullptr);
  });
}

// Partial decryption of K ciphertexts [K][2][towers][N] with the context's key share and smudging
// noise (threshold.hip); the noise stream advances by K.  The caller holds ctx->mu, has selected the
// device and checked the keys.  Synchronises s (the noise's scratch is reused by the next call).
void partial_decrypt_locked(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, uint32_t towers, bool lead,
                            uint64_t* out_dev, hipStream_t s) {
  const Params& p = ctx->p;
  if (towers < 1 || towers > p.L) throw Error{SHELFI_ERR_ARG, "tower count out of range for this context"};
  if (!K) return;
  const double sigma = ctx->thr_sigma;
  uint32_t key[8] = {};
  KeyWiper wipe(key);
  const uint64_t g0 = ctx->thr_counter;
  ctx->thr_counter += K;
  if (sigma > 0.0) {
    if (ctx->seed)
      seed_to_key(ctx->seed, key);
    else
      os_random(key, 32);
  }
  const size_t per_ct = partial_decrypt_scratch_bytes(p, towers, 1, sigma);
  const uint64_t kc_max = per_ct ? dev_chunk(K, per_ct) : K;
  void* scratch = per_ct ? ensure(ctx->scratch, ctx->scratch_bytes, per_ct * kc_max) : nullptr;
  const size_t tn = (size_t)towers * p.N;
  for (uint64_t k0 = 0; k0 < K; k0 += kc_max) {
    const uint64_t kc = std::min<uint64_t>(kc_max, K - k0);
    launch_partial_decrypt(p, ctx->dt, ctx->dk, ct_dev + k0 * 2 * tn, kc, towers, lead, out_dev + k0 * tn, scratch,
                           sigma, key, g0 + k0, s);
  }
  SHELFI_HIP(hipStreamSynchronize(s));
}

}  // namespace shelfi

extern "C" {

int shelfi_dev_wavg(shelfi_ctx* ctx, const uint64_t* const* in_dev, const float* w, size_t C,
                    size_t K, uint64_t* out_dev, void* stream) {
  if (!ctx || !out_dev || (C && (!in_dev || !w))) return SHELFI_ERR_ARG;
  return guarded([&] {
    if (!C) throw Error{SHELFI_ERR_ARG, "no learners"};
    check_wavg_weights(w, C, ctx->p.delta);
    DeviceGuard g(ctx->device);
    const Params& p = ctx->p;
    hipStream_t s = (hipStream_t)stream;  // 0 = legacy default stream
    for (size_t c0 = 0; c0 < C; c0 += kWavgMaxLearners) {
      const size_t gc = std::min<size_t>(kWavgMaxLearners, C - c0);
      WavgArgs a;
      std::memset(&a, 0, sizeof(a));
      for (size_t c = 0; c < gc; ++c) a.ptrs[c] = in_dev[c0 + c];
      fill_weights(a, p, w + c0, gc);
      a.out = out_dev;
      a.rows = (uint64_t)K * 2 * p.L;
      a.C = (uint32_t)gc;
      a.L = p.L;
      a.logN = p.logN;
      a.accumulate = c0 ? 1 : 0;
      launch_wavg(a, ctx->dt.tc, s);
    }
  });
}

int shelfi_dev_check_residues(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, void* stream) {
  if (!ctx || (K && !ct_dev)) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    if (!K) return;
    DeviceGuard g(ctx->device);
    const Params& p = ctx->p;
    hipStream_t s = (hipStream_t)stream;
    uint32_t* bad = ctx->dev_flag + 6;
    SHELFI_HIP(hipMemsetAsync(bad, 0, 4, s));
    launch_check_residues(ct_dev, (uint64_t)K * 2 * p.L, p.L, p.logN, ctx->dt.tc, bad, s);
    SHELFI_HIP(hipMemcpyAsync(ctx->host_flag + 6, bad, 4, hipMemcpyDeviceToHost, s));
    SHELFI_HIP(hipStreamSynchronize(s));
    if (ctx->host_flag[6])
      throw Error{SHELFI_ERR_FORMAT, "ciphertext residue >= its tower modulus (malformed batch)"};
  });
}

size_t shelfi_arena_words(const shelfi_ctx* ctx, size_t C, size_t K) {
  if (!ctx) return 0;
  return (size_t)arena_ct_words(ctx->p, C) * K;
}

int shelfi_dev_arena_put(shelfi_ctx* ctx, const void* src, int src_on_host, size_t K, size_t learner,
                         size_t C, uint64_t* arena_dev, void* stream) {
  if (!ctx || !arena_dev || (K && !src) || learner >= C) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    DeviceGuard g(ctx->device);
    if (!K) return;
    const Params& p = ctx->p;
    hipStream_t s = (hipStream_t)stream;
    const size_t ct_words = 2ull * p.L * p.N;
    if (!src_on_host) {
      arena_place(ctx, K, learner, C, arena_dev, s, K, false, [&](size_t k0, size_t, uint64_t*) {
        return (const uint64_t*)src + k0 * ct_words;
      });
      return;
    }
    // host batches go through the pinned staging ring (the bytes API's copy pool)
    StageRun sr(stager(ctx));
    arena_place(ctx, K, learner, C, arena_dev, s, arena_stage_cts(p), true, [&](size_t k0, size_t kn, uint64_t* dst) {
      if (!arena_use_stager(1, kn * ct_words * 8)) {
        SHELFI_HIP(hipMemcpyAsync(dst, (const uint64_t*)src + k0 * ct_words, kn * ct_words * 8,
                                  hipMemcpyHostToDevice, s));
      } else {
        const HostPiece pc{(uint8_t*)((const uint64_t*)src + k0 * ct_words), kn * ct_words * 8};
        sr.s.h2dv(dst, &pc, 1, s);
      }
      return (const uint64_t*)dst;
    });
    sr.finish();
  });
}

int shelfi_dev_arena_put_blob(shelfi_ctx* ctx, const uint8_t* blob, size_t len, size_t K, size_t learner,
                              size_t C, uint64_t* arena_dev, void* stream) {
  if (!ctx || !arena_dev || !blob || learner >= C) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    // header first, against the context (parameters, key tag / key id), before any copy; a
    // refused header marks the slot refused too, so the slot's previous round cannot be
    // aggregated as if this upload had landed (the residue check below does the same)
    CtLayout v;
    try {
      v = open_cts(ctx, blob, len);
      if (v.K != K)
        throw Error{SHELFI_ERR_FORMAT, "upload holds " + std::to_string(v.K) + " ciphertexts, the arena " +
                                           std::to_string(K)};
    } catch (...) {
      arena_mark(ctx, arena_dev, (size_t)arena_ct_words(ctx->p, C) * K, C, learner, true);
      throw;
    }
    if (!K) return;
    DeviceGuard g(ctx->device);
    const Params& p = ctx->p;
    hipStream_t s = (hipStream_t)stream;
    std::vector<HostPiece> pcs;
    StageRun sr(stager(ctx));
    // a packed blob lands packed (in the bytes-API buffer, idle under the ctx lock) and is unpacked
    const uint64_t pct = 2 * packed_poly_bytes(p, p.L);
    uint8_t* pk = v.packed ? (uint8_t*)ensure(ctx->io, ctx->io_bytes, std::min(K, arena_stage_cts(p)) * pct) : nullptr;
    const ArenaPack ap = arena_pack(p);
    arena_place(ctx, K, learner, C, arena_dev, s, arena_stage_cts(p), true, [&](size_t k0, size_t kn, uint64_t* dst) {
      // a blob: one payload run; an archive: 2 L tower runs per ciphertext
      v.pieces(k0, kn, p, pcs);
      uint8_t* land = v.packed ? pk : (uint8_t*)dst;
      size_t bytes = 0;
      for (const HostPiece& pc : pcs) bytes += pc.n;
      if (arena_use_stager(pcs.size(), bytes)) {
        sr.s.h2dv(land, pcs.data(), pcs.size(), s);  // pinned staging ring, gathered in order
      } else {
        uint8_t* d = land;
        for (const HostPiece& pc : pcs) {
          SHELFI_HIP(hipMemcpyAsync(d, pc.p, pc.n, hipMemcpyHostToDevice, s));
          d += pc.n;
        }
      }
      if (v.packed) launch_blob_unpack((const uint32_t*)pk, kn, p.L, p.logN, ap, dst, s);
      return (const uint64_t*)dst;
    });
    sr.finish();
  });
}

int shelfi_dev_arena_release(shelfi_ctx* ctx, const uint64_t* arena_dev, size_t words) {
  if (!ctx || (words && !arena_dev)) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    auto& R = ctx->arena_refused;
    for (size_t i = 0; i < R.size();)
      if (arena_dev < R[i].arena + R[i].words && R[i].arena < arena_dev + words) R.erase(R.begin() + (long)i);
      else ++i;
  });
}

int shelfi_dev_wavg_arena(shelfi_ctx* ctx, const uint64_t* arena_dev, const float* w, size_t C,
                          size_t K, uint64_t* out_dev, void* stream) {
  if (!ctx || !out_dev || (C && (!arena_dev || !w))) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    if (!C) throw Error{SHELFI_ERR_ARG, "no learners"};
    check_wavg_weights(w, C, ctx->p.delta);
    arena_require_valid_locked(ctx, arena_dev, (size_t)arena_ct_words(ctx->p, C) * K);
    DeviceGuard g(ctx->device);
    wavg_arena_enqueue(ctx, arena_dev, w, C, K, out_dev, (hipStream_t)stream);
  });
}

int shelfi_dev_wavg_arena_packed(shelfi_ctx* ctx, const uint64_t* arena_dev, const float* w, size_t C, size_t K,
                                 uint64_t* out_packed, void* stream) {
  if (!ctx || (K && !out_packed) || (C && (!arena_dev || !w))) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    if (!C) throw Error{SHELFI_ERR_ARG, "no learners"};
    check_wavg_weights(w, C, ctx->p.delta);
    arena_require_valid_locked(ctx, arena_dev, (size_t)arena_ct_words(ctx->p, C) * K);
    DeviceGuard g(ctx->device);
    wavg_arena_enqueue_packed(ctx, arena_dev, w, C, K, out_packed, (hipStream_t)stream);
  });
}

int shelfi_dev_sum_packed(shelfi_ctx* ctx, const uint64_t* stacked, size_t G, size_t K, size_t stride_words,
                          uint64_t* out_dev, void* stream) {
  if (!ctx || (K && (!stacked || !out_dev))) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    DeviceGuard g(ctx->device);
    sum_packed_enqueue(ctx, stacked, G, K, stride_words, out_dev, (hipStream_t)stream);
  });
}

int shelfi_dev_wavg_arena_pick_output(shelfi_ctx* ctx, const uint64_t* arena_dev, const float* w,
                                      size_t C, size_t K, uint64_t* const* candidates, size_t n,
                                      int launches, size_t* best, float* ms, void* stream) {
  if (!ctx || !candidates || !best || !n || launches < 1) return SHELFI_ERR_ARG;
  return guarded([&] {
    DeviceGuard g(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    struct Events {
      hipEvent_t a = nullptr, b = nullptr;
      ~Events() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
      }
    } ev;
    SHELFI_HIP(hipEventCreate(&ev.a));
    SHELFI_HIP(hipEventCreate(&ev.b));
    auto run = [&](uint64_t* out) {
      const int rc = shelfi_dev_wavg_arena(ctx, arena_dev, w, C, K, out, stream);
      if (rc) throw Error{rc, shelfi_last_error()};
    };
    float best_ms = 0.f;
    for (size_t i = 0; i < n; ++i) {
      if (!candidates[i]) throw Error{SHELFI_ERR_ARG, "null candidate buffer"};
      run(candidates[i]);  // warm-up
      SHELFI_HIP(hipEventRecord(ev.a, s));
      for (int l = 0; l < launches; ++l) run(candidates[i]);
      SHELFI_HIP(hipEventRecord(ev.b, s));
      SHELFI_HIP(hipEventSynchronize(ev.b));
      float t = 0.f;
      SHELFI_HIP(hipEventElapsedTime(&t, ev.a, ev.b));
      t /= (float)launches;
      if (ms) ms[i] = t;
      if (i == 0 || t < best_ms) {
        best_ms = t;
        *best = i;
      }
    }
  });
}

int shelfi_dev_modq(shelfi_ctx* ctx, uint64_t* buf_dev, size_t K, void* stream) {
  if (!ctx || !buf_dev) return SHELFI_ERR_ARG;
  return guarded([&] {
    DeviceGuard g(ctx->device);
    hipStream_t s = (hipStream_t)stream;  // 0 = legacy default stream
    launch_modq(buf_dev, (uint64_t)K * 2 * ctx->p.L, ctx->p.L, ctx->p.logN, ctx->dt.tc, s);
  });
}

int shelfi_dev_encrypt(shelfi_ctx* ctx, const double* x_dev, size_t n, uint64_t* ct_dev,
                       void* stream) {
  if (!ctx || (n && (!x_dev || !ct_dev))) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    require_keys(ctx);
    DeviceGuard g(ctx->device);
    const Params& p = ctx->p;
    hipStream_t s = (hipStream_t)stream;  // 0 = legacy default stream
    const uint64_t K = (n + p.batch - 1) / p.batch;
    if (!K) return;
    uint32_t key[8];
    KeyWiper wipe(key);
    uint64_t g0;
    draw_key(ctx, K, key, &g0);
    const uint64_t kc_max = dev_chunk(K, encrypt_scratch_bytes(p, 1));
    void* scratch = ensure(ctx->scratch, ctx->scratch_bytes, encrypt_scratch_bytes(p, kc_max));
    const GenFlag fl = next_gen_flag(ctx);
    const size_t ct_words = 2ull * p.L * p.N;
    bool approx = false;
    for (int pass = 0; pass < 2; ++pass) {
      for (uint64_t k0 = 0; k0 < K; k0 += kc_max) {
        const uint64_t kc = std::min(kc_max, K - k0);
        const uint64_t xs = k0 * p.batch, xn = std::min<uint64_t>(n - xs, kc * p.batch);
        if (approx)
          launch_encrypt_approx(p, ctx->dt, ctx->dk, x_dev + xs, xn, kc, ct_dev + k0 * ct_words, scratch, key,
                                g0 + k0, s);
        else
          launch_encrypt(p, ctx->dt, ctx->dk, x_dev + xs, xn, kc, ct_dev + k0 * ct_words, scratch,
                         key, g0 + k0, fl, s);
      }
      if (approx) break;
      SHELFI_HIP(hipStreamSynchronize(s));  // scratch is reused by the next call
      if (!encode_needs_approx(ctx, fl)) break;
      approx = true;  // some message coefficient above 2^61: redo the call on the large-value path
      ++ctx->encode_redo_count;
    }
  });
}

int shelfi_dev_decrypt(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, double scale, size_t n,
                       double* out_dev, void* stream) {
  return dev_decrypt(ctx, ct_dev, K, ctx ? ctx->p.L : 0, scale, n, out_dev, stream);
}

// ---- plaintext operands (plain.hip) ----
int shelfi_dev_encode(shelfi_ctx* ctx, const double* x_dev, size_t n, uint32_t towers, double scale,
                      uint64_t* pt_dev, void* stream) {
  if (!ctx || (n && (!x_dev || !pt_dev))) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    const Params& p = ctx->p;
    if (towers < 1 || towers > p.L) throw Error{SHELFI_ERR_ARG, "tower count out of range for this context"};
    if (!(scale > 0.0) || !std::isfinite(scale)) throw Error{SHELFI_ERR_ARG, "encode: the scale must be finite and positive"};
    const uint64_t K = (n + p.batch - 1) / p.batch;
    if (!K) return;
    DeviceGuard g(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    const uint64_t kc_max = dev_chunk(K, encode_scratch_bytes(p, 1));
    void* scratch = ensure(ctx->scratch, ctx->scratch_bytes, encode_scratch_bytes(p, kc_max));
    const GenFlag fl = next_gen_flag(ctx);  // the call's own generation of the range words
    const size_t pt_words = (size_t)towers * p.N;
    for (uint64_t k0 = 0; k0 < K; k0 += kc_max) {
      const uint64_t kc = std::min(kc_max, K - k0);
      const uint64_t xs = k0 * p.batch, xn = std::min<uint64_t>(n - xs, kc * p.batch);
      launch_encode_plain(p, ctx->dt, x_dev + xs, xn, kc, towers, scale, pt_dev + k0 * pt_words, scratch, fl, s);
    }
    SHELFI_HIP(hipStreamSynchronize(s));  // scratch is reused by the next call; the range words are final
    if (gen_flag_raised(ctx, fl, 1)) throw Error{SHELFI_ERR_RANGE, "encode: non-finite input value"};
    if (gen_flag_raised(ctx, fl, 0))
      throw Error{SHELFI_ERR_RANGE, "encode: a coefficient |x * scale| above 2^61 (the plaintext encode has no large-value path)"};
  });
}

namespace {
bool words_overlap(const uint64_t* a, const uint64_t* b, uint64_t na, uint64_t nb) { return a < b + nb && b < a + na; }

// the three ciphertext-with-plaintext calls: op as launch_plain_op takes it
int dev_plain_op(int op, shelfi_ctx* ctx, const uint64_t* ct_dev, const uint64_t* pt_dev, size_t K, size_t Kp,
                 uint32_t towers, uint64_t* out_dev, void* stream) {
  if (!ctx || (K && (!ct_dev || !pt_dev || !out_dev))) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    const Params& p = ctx->p;
    if (towers < 1 || towers > p.L) throw Error{SHELFI_ERR_ARG, "tower count out of range for this context"};
    if (!K) return;
    if (Kp != 1 && Kp != K) throw Error{SHELFI_ERR_ARG, "plaintext operand: one plaintext per ciphertext, or one for all"};
    // each thread reads its residues before writing them: out may be ct exactly, not shifted
    const uint64_t cw = 2ull * towers * p.N * K, pw = (uint64_t)towers * p.N * Kp;
    if ((out_dev != ct_dev && words_overlap(ct_dev, out_dev, cw, cw)) || words_overlap(pt_dev, out_dev, pw, cw))
      throw Error{SHELFI_ERR_ARG, "plaintext operand: the output must be the ciphertext input exactly or overlap no input"};
    DeviceGuard g(ctx->device);
    launch_plain_op(op, ct_dev, pt_dev, K, Kp, towers, p.logN, ctx->dt.tc, out_dev, (hipStream_t)stream);
  });
}

// EvalSub (b_dev set) and EvalNegate (b_dev null)
int dev_ct_sub(shelfi_ctx* ctx, const uint64_t* a_dev, const uint64_t* b_dev, bool neg, size_t K, uint32_t towers,
               uint64_t* out_dev, void* stream) {
  if (!ctx || (K && (!a_dev || (!neg && !b_dev) || !out_dev))) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    const Params& p = ctx->p;
    if (towers < 1 || towers > p.L) throw Error{SHELFI_ERR_ARG, "tower count out of range for this context"};
    if (!K) return;
    const uint64_t words = 2ull * towers * p.N * K;
    for (const uint64_t* in : {a_dev, b_dev})
      if (in && out_dev != in && words_overlap(in, out_dev, words, words))
        throw Error{SHELFI_ERR_ARG, "EvalSub / EvalNegate output must be an input exactly or not overlap the inputs"};
    DeviceGuard g(ctx->device);
    launch_ct_sub(a_dev, neg ? nullptr : b_dev, K * 2 * towers, towers, p.logN, ctx->dt.tc, out_dev, (hipStream_t)stream);
  });
}
}  // namespace

int shelfi_dev_mult_plain(shelfi_ctx* ctx, const uint64_t* ct_dev, const uint64_t* pt_dev, size_t K, size_t Kp,
                          uint32_t towers, uint64_t* out_dev, void* stream) {
  return dev_plain_op(0, ctx, ct_dev, pt_dev, K, Kp, towers, out_dev, stream);
}
int shelfi_dev_add_plain(shelfi_ctx* ctx, const uint64_t* ct_dev, const uint64_t* pt_dev, size_t K, size_t Kp,
                         uint32_t towers, uint64_t* out_dev, void* stream) {
  return dev_plain_op(1, ctx, ct_dev, pt_dev, K, Kp, towers, out_dev, stream);
}
int shelfi_dev_sub_plain(shelfi_ctx* ctx, const uint64_t* ct_dev, const uint64_t* pt_dev, size_t K, size_t Kp,
                         uint32_t towers, uint64_t* out_dev, void* stream) {
  return dev_plain_op(2, ctx, ct_dev, pt_dev, K, Kp, towers, out_dev, stream);
}
int shelfi_dev_sub(shelfi_ctx* ctx, const uint64_t* a_dev, const uint64_t* b_dev, size_t K, uint32_t towers,
                   uint64_t* out_dev, void* stream) {
  return dev_ct_sub(ctx, a_dev, b_dev, false, K, towers, out_dev, stream);
}
int shelfi_dev_negate(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, uint32_t towers, uint64_t* out_dev,
                      void* stream) {
  return dev_ct_sub(ctx, ct_dev, nullptr, true, K, towers, out_dev, stream);
}

int shelfi_dev_decrypt_level(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, uint32_t towers, double scale,
                             size_t n, double* out_dev, void* stream) {
  return dev_decrypt(ctx, ct_dev, K, towers, scale, n, out_dev, stream);
}

int shelfi_dev_decrypt_sum(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, uint32_t terms, double scale,
                           size_t n, double* out_dev, void* stream) {
  if (terms < 1 || terms > (uint32_t)kMaxCommRanks) {
    set_error("decrypt_sum: the residues must be sums of 1..16 canonical residues");
    return SHELFI_ERR_ARG;
  }
  return dev_decrypt(ctx, ct_dev, K, ctx ? ctx->p.L : 0, scale, n, out_dev, stream, true);
}

int shelfi_dev_partial_decrypt(shelfi_ctx* ctx, const uint64_t* ct_dev, size_t K, uint32_t towers, int lead,
                               uint64_t* out_dev, void* stream) {
  if (!ctx || (K && (!ct_dev || !out_dev))) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    require_keys(ctx);
    DeviceGuard g(ctx->device);
    partial_decrypt_locked(ctx, ct_dev, K, towers, lead != 0, out_dev, (hipStream_t)stream);
  });
}

int shelfi_dev_fuse_decrypt(shelfi_ctx* ctx, const uint64_t* const* partials_dev, size_t P, size_t K,
                            uint32_t towers, double scale, size_t n, double* out_dev, void* stream) {
  if (!ctx || (n && !out_dev)) return SHELFI_ERR_ARG;
  if (!partials_dev || P < 1 || P > (size_t)kMaxCommRanks) {
    set_error("fuse_decrypt: 1..16 partial decryptions");
    return SHELFI_ERR_ARG;
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    FuseIn fz{};
    fz.P = (uint32_t)P;
    for (size_t i = 0; i < P; ++i) {
      if (n && !partials_dev[i]) throw Error{SHELFI_ERR_ARG, "fuse_decrypt: null partial"};
      fz.part[i] = partials_dev[i];
    }
    DeviceGuard g(ctx->device);
    dev_decrypt_locked(ctx, nullptr, K, towers, scale, n, out_dev, (hipStream_t)stream, false, &fz);
  });
}

int shelfi_dev_ntt(shelfi_ctx* ctx, uint64_t* polys_dev, size_t P, int inverse, void* stream) {
  if (!ctx || (P && !polys_dev)) return SHELFI_ERR_ARG;
  return guarded([&] {
    DeviceGuard g(ctx->device);
    hipStream_t s = (hipStream_t)stream;  // 0 = legacy default stream
    launch_ntt(polys_dev, P, ctx->p.L, ctx->p.logN, inverse != 0, ctx->dt, s);
  });
}

}  // extern "C"
