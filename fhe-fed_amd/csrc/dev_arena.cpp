// dev_arena.cpp — the packed resident arena of the device API: uploads placed into their packed
// slices with the canonical-residue check riding along (shelfi_dev_arena_put*), the refused-slot bookkeeping,
// and the aggregations that read the arena (shelfi_dev_wavg_arena*, shelfi_dev_sum_packed).
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
  const size_t bytes = wl.size() * sizeof(uint32_t);
  const int i = weight_ring_slot(ctx, bytes);
  ctx->wl_host[i] = std::move(wl);  // stays alive until the slot is reused
  SHELFI_HIP(hipMemcpyAsync(ctx->wl_dev[i], ctx->wl_host[i].data(), bytes, hipMemcpyHostToDevice, s));
  return ctx->wl_last_slot = i;
}

// The ring itself, for any small table a kernel reads (the weight limbs above, EvalPoly's constants): the next
// slot, waited for if the kernels that read it last are still running, grown to `bytes` if need be.  The caller
// fills wl_dev[slot] by a copy ordered on its stream and records wl_done[slot] behind the kernels that read it.
int weight_ring_slot(shelfi_ctx* ctx, size_t bytes) {
  const int i = ctx->wl_next;
  ctx->wl_next = (i + 1) % shelfi_ctx::kWeightRing;
  if (ctx->wl_done[i]) SHELFI_HIP(hipEventSynchronize(ctx->wl_done[i]));
  else SHELFI_HIP(hipEventCreateWithFlags(&ctx->wl_done[i], hipEventDisableTiming));
  if (ctx->wl_cap[i] < bytes) {
    if (ctx->wl_dev[i]) (void)hipFree(ctx->wl_dev[i]);
    ctx->wl_dev[i] = nullptr;
    ctx->wl_cap[i] = 0;
    SHELFI_HIP(hipMalloc(&ctx->wl_dev[i], bytes));
    ctx->wl_cap[i] = bytes;
  }
  if (ctx->wl_last_slot == i) ctx->wl_last_slot = -1;  // (the slot's weights are about to be replaced)
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
    const bool overlaps = words_overlap(arena, words, r.arena, r.words);
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
    if (words_overlap(a, words, r.arena, r.words))
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

}  // namespace shelfi

extern "C" {

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
    // (a seeded blob's c0 groups the same way; c1 is expanded beside them)
    const bool vp = v.packed || v.seeded;
    const uint64_t pct = (v.seeded ? 1 : 2) * packed_poly_bytes(p, p.L);
    uint8_t* pk = vp ? (uint8_t*)ensure(ctx->io, ctx->io_bytes, std::min(K, arena_stage_cts(p)) * pct) : nullptr;
    const ArenaPack ap = arena_pack(p);
    arena_place(ctx, K, learner, C, arena_dev, s, arena_stage_cts(p), true, [&](size_t k0, size_t kn, uint64_t* dst) {
      // a blob: one payload run; an archive: 2 L tower runs per ciphertext
      v.pieces(k0, kn, p, pcs);
      uint8_t* land = vp ? pk : (uint8_t*)dst;
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
      if (v.seeded) seeded_land(ctx, v, pk, k0, kn, p.L, ap, dst, s);
      return (const uint64_t*)dst;
    });
    sr.finish();
  });
}

// Any ciphertext bytes -> the uint64 batch [K][2][L][N] on the device: a uint64 blob or an archive copied, a
// packed blob unpacked, a seeded blob's c0 unpacked and its c1 expanded (seeded.hip); the header is checked
// against the context first and the landed residues against their moduli after.
int shelfi_dev_blob_unpack(shelfi_ctx* ctx, const uint8_t* blob, size_t len, size_t K, uint64_t* out_dev,
                           void* stream) {
  if (!ctx || !blob || (K && !out_dev)) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    const CtLayout v = open_cts(ctx, blob, len);
    if (v.K != K)
      throw Error{SHELFI_ERR_FORMAT, "blob holds " + std::to_string(v.K) + " ciphertexts, the output " +
                                         std::to_string(K)};
    if (!K) return;
    DeviceGuard g(ctx->device);
    const Params& p = ctx->p;
    hipStream_t s = (hipStream_t)stream;
    const size_t ct_words = 2ull * p.L * p.N, kc = arena_stage_cts(p);
    const bool vp = v.packed || v.seeded;
    const uint64_t pct = (v.seeded ? 1 : 2) * packed_poly_bytes(p, p.L);
    uint8_t* pk = vp ? (uint8_t*)ensure(ctx->io, ctx->io_bytes, std::min(K, kc) * pct) : nullptr;
    const ArenaPack ap = arena_pack(p);
    std::vector<HostPiece> pcs;
    StageRun sr(stager(ctx));
    for (size_t k0 = 0; k0 < K; k0 += kc) {
      const size_t kn = std::min(kc, K - k0);
      uint64_t* dst = out_dev + k0 * ct_words;
      v.pieces(k0, kn, p, pcs);
      sr.s.h2dv(vp ? pk : (uint8_t*)dst, pcs.data(), pcs.size(), s);
      if (v.packed) launch_blob_unpack((const uint32_t*)pk, kn, p.L, p.logN, ap, dst, s);
      if (v.seeded) seeded_land(ctx, v, pk, k0, kn, p.L, ap, dst, s);
    }
    uint32_t* bad = ctx->dev_flag + 6;
    SHELFI_HIP(hipMemsetAsync(bad, 0, 4, s));
    launch_check_residues(out_dev, (uint64_t)K * 2 * p.L, p.L, p.logN, ctx->dt.tc, bad, s);
    SHELFI_HIP(hipMemcpyAsync(ctx->host_flag + 6, bad, 4, hipMemcpyDeviceToHost, s));
    sr.finish();
    SHELFI_HIP(hipStreamSynchronize(s));
    if (ctx->host_flag[6])
      throw Error{SHELFI_ERR_FORMAT, "ciphertext residue >= its tower modulus (malformed batch)"};
  });
}

int shelfi_dev_arena_release(shelfi_ctx* ctx, const uint64_t* arena_dev, size_t words) {
  if (!ctx || (words && !arena_dev)) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    auto& R = ctx->arena_refused;
    for (size_t i = 0; i < R.size();)
      if (words_overlap(arena_dev, words, R[i].arena, R[i].words)) R.erase(R.begin() + (long)i);
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

}  // extern "C"
