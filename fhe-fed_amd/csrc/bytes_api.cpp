// bytes_api.cpp — the bytes API (host buffers in, host buffers out): encrypt, weighted average and
// decrypt as three-stream pipelines over chunks of the call.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "api_internal.h"
#include "api_util.h"

using namespace shelfi;

namespace shelfi {

// Three-stage pipeline over chunks: H2D on stream A, kernels on stream B (scratch is
// reused chunk after chunk on B), D2H on stream C, two staging buffer sets.
struct Pipe {
  hipStream_t a, b, c;
  hipEvent_t in_ready[2], computed[2], out_free[2];
  explicit Pipe(shelfi_ctx* ctx) : a(ctx->stream), b(ctx->stream2), c(ctx->stream3) {
    for (int i = 0; i < 2; ++i) {
      in_ready[i] = computed[i] = out_free[i] = nullptr;
    }
    for (int i = 0; i < 2; ++i) {
      SHELFI_HIP(hipEventCreateWithFlags(&in_ready[i], hipEventDisableTiming));
      SHELFI_HIP(hipEventCreateWithFlags(&computed[i], hipEventDisableTiming));
      SHELFI_HIP(hipEventCreateWithFlags(&out_free[i], hipEventDisableTiming));
    }
  }
  ~Pipe() {
    (void)hipStreamSynchronize(c);  // no-ops on success; on an error, nothing stays in flight
    (void)hipStreamSynchronize(b);
    (void)hipStreamSynchronize(a);
    for (int i = 0; i < 2; ++i) {
      if (in_ready[i]) (void)hipEventDestroy(in_ready[i]);
      if (computed[i]) (void)hipEventDestroy(computed[i]);
      if (out_free[i]) (void)hipEventDestroy(out_free[i]);
    }
  }
  void sync() {
    SHELFI_HIP(hipStreamSynchronize(c));
    SHELFI_HIP(hipStreamSynchronize(b));
    SHELFI_HIP(hipStreamSynchronize(a));
  }
};

// The ctx's pinned staging rings (8 slots each way, SHELFI_STAGE_SLOT_MIB each), created on first use
// and re-created between calls when the slot size switch changes (the ring is idle then).  16 MiB: a
// bytes-API learner chunk (4 cts, 8 MiB + its archive headers) is one DMA; pinned copies of 8 / 16 / 32
// MiB ran 53.5 / 55.4 / 56.3 GB/s (profiles/r05u/pinned_h2d.json) and the archive aggregation 45.1 -> 48.4
// GB/s with 16 MiB slots, the other bytes-API rates within noise (profiles/r05u/bench_slot*).
Stager& stager(shelfi_ctx* ctx) {
  const size_t slot = (size_t)switches().stage_slot_mib << 20;
  if (ctx->stage && ctx->stage->slot_bytes() != slot) {
    delete ctx->stage;
    ctx->stage = nullptr;
  }
  if (!ctx->stage) ctx->stage = new Stager(slot, 8, 8, default_copy_threads());
  return *ctx->stage;
}

// encode + encrypt n doubles (host) -> K ciphertext payloads written to out_payload (approx: every
// chunk on the large-value path, launch_encrypt_approx; same key and counters, so the same samples).
static void encrypt_bytes_pipeline(shelfi_ctx* ctx, const double* x, size_t n, uint64_t K,
                                   const CtLayout& dst, const uint32_t key[8], uint64_t g0, bool approx) {
  const Params& p = ctx->p;
  const size_t ct_bytes = 2ull * p.L * p.N * 8;
  uint64_t kc = std::max<uint64_t>(1, (64ull << 20) / ct_bytes);
  kc = std::min<uint64_t>(kc, K);
  const size_t xin = kc * values_per_ct(p) * 8, cto = kc * ct_bytes;
  // packed wire output: the chunk is packed on the device (U_t bits per residue) before its D2H
  // seeded wire output: the symmetric encrypt's c0 [kc][L][N] takes the chunk's uint64 buffer and is packed
  // one group a ciphertext
  const size_t pko = dst.packed ? kc * 2 * packed_poly_bytes(p, p.L) : dst.seeded ? kc * packed_poly_bytes(p, p.L) : 0;
  uint8_t* io = (uint8_t*)ensure(ctx->io, ctx->io_bytes, 2 * (xin + cto + pko));
  uint8_t* xb[2] = {io, io + xin};
  uint8_t* cb[2] = {io + 2 * xin, io + 2 * xin + cto};
  uint8_t* pb[2] = {io + 2 * (xin + cto), io + 2 * (xin + cto) + pko};
  const ArenaPack ap = arena_pack(p);
  void* scratch = ensure(ctx->scratch, ctx->scratch_bytes,
                         dst.seeded ? seeded_encrypt_scratch_bytes(p, kc) : encrypt_scratch_bytes(p, kc));
  Pipe pp(ctx);
  StageRun sr(stager(ctx));
  std::vector<HostPiece> pcs;
  const GenFlag fl = next_gen_flag(ctx);
  const uint64_t nchunks = (K + kc - 1) / kc;
  for (uint64_t ci = 0; ci < nchunks; ++ci) {
    const int b = (int)(ci & 1);
    const uint64_t k0 = ci * kc, kn = std::min<uint64_t>(kc, K - k0);
    const uint64_t xs = k0 * values_per_ct(p), xn = std::min<uint64_t>(n - xs, kn * values_per_ct(p));
    if (ci >= 2) SHELFI_HIP(hipStreamWaitEvent(pp.a, pp.computed[b], 0));  // x buffer consumed
    sr.s.h2d(xb[b], x + xs, xn * 8, pp.a);
    SHELFI_HIP(hipEventRecord(pp.in_ready[b], pp.a));
    SHELFI_HIP(hipStreamWaitEvent(pp.b, pp.in_ready[b], 0));
    if (ci >= 2) SHELFI_HIP(hipStreamWaitEvent(pp.b, pp.out_free[b], 0));  // ct buffer drained
    if (dst.seeded)
      launch_encrypt_seeded(p, ctx->dt, ctx->dk, (const double*)xb[b], xn, kn, (uint64_t*)cb[b], scratch, key,
                            g0 + k0, dst.seed, k0, fl, pp.b);
    else if (approx)
      launch_encrypt_approx(p, ctx->dt, ctx->dk, (const double*)xb[b], xn, kn, (uint64_t*)cb[b], scratch, key,
                            g0 + k0, pp.b);
    else
      launch_encrypt(p, ctx->dt, ctx->dk, (const double*)xb[b], xn, kn, (uint64_t*)cb[b], scratch, key,
                     g0 + k0, fl, pp.b);
    if (dst.packed)  // canonical residues: the residue check cannot fire
      launch_blob_pack((const uint64_t*)cb[b], kn, p.L, p.logN, ap, ctx->dt.tc, (uint32_t*)pb[b],
                       ctx->dev_flag + 5, pp.b);
    if (dst.seeded)  // kn groups of L towers: the rows of kn polynomials
      launch_arena_pack((const uint64_t*)cb[b], 0, kn * p.L << (p.logN - 9), 1, 0, p.L, p.logN, ap, ctx->dt.tc,
                        (uint64_t*)pb[b], ctx->dev_flag + 5, pp.b);
    SHELFI_HIP(hipEventRecord(pp.computed[b], pp.b));
    SHELFI_HIP(hipStreamWaitEvent(pp.c, pp.computed[b], 0));
    dst.pieces(k0, kn, p, pcs);
    sr.s.d2hv(pcs.data(), pcs.size(), dst.packed || dst.seeded ? pb[b] : cb[b], pp.c);
    SHELFI_HIP(hipEventRecord(pp.out_free[b], pp.c));
    sr.s.poll();
  }
  sr.finish();
  pp.sync();
  if (dst.seeded) {  // the symmetric encrypt has no large-value path
    if (gen_flag_raised(ctx, fl, 1)) throw Error{SHELFI_ERR_RANGE, "encrypt (seeded): non-finite input value"};
    if (gen_flag_raised(ctx, fl, 0))
      throw Error{SHELFI_ERR_RANGE, "encrypt (seeded): a coefficient |x * scale| above 2^61 (the symmetric encrypt has no large-value path)"};
    return;
  }
  if (!approx && encode_needs_approx(ctx, fl)) {  // once per call, whichever chunks were flagged
    ++ctx->encode_redo_count;
    encrypt_bytes_pipeline(ctx, x, n, K, dst, key, g0, true);
  }
}

// Validates the learners' batches (same format, params, key, K, depth, scale).
static std::vector<CtLayout> wavg_inputs(const shelfi_ctx* ctx, const uint8_t* const* blobs,
                                         const size_t* lens, size_t C) {
  if (C == 0) throw Error{SHELFI_ERR_ARG, "computeWeightedAverage: no learners"};
  std::vector<CtLayout> in;
  in.reserve(C);
  for (size_t c = 0; c < C; ++c) {
    in.push_back(open_cts(ctx, blobs[c], lens[c]));
    const CtLayout& h = in.back();
    const CtLayout& h0 = in.front();
    if (h.pal != h0.pal)
      throw Error{SHELFI_ERR_FORMAT, "learners mix PALISADE archives and library blobs"};
    if (h.seeded != h0.seeded)
      throw Error{SHELFI_ERR_FORMAT, "learners mix seeded and other library blobs"};
    if (h.packed != h0.packed)
      throw Error{SHELFI_ERR_FORMAT, "learners mix packed and uint64 library blobs"};
    if (h.K != h0.K)
      throw Error{SHELFI_ERR_FORMAT, "learners hold different numbers of ciphertexts"};
    if (h.depth != h0.depth || h.scale != h0.scale || h.level != h0.level)
      throw Error{SHELFI_ERR_FORMAT, "learners' ciphertexts have different depth/scale"};
  }
  return in;
}

// Pipelined bytes -> bytes aggregation: the K ciphertexts are processed in chunks;
// chunk i's H2D copies (all learners, stream A) overlap chunk i-1's wavg + D2H
// (stream B), with two device buffer sets.  Writes the payload of the result.
// Uploads (round 5): each learner's chunk is one contiguous byte range of its blob -- a PALISADE
// archive's range (tower headers included) lands raw and its tower runs are gathered into [K][2][L][N]
// on the device.  By default the range goes through the pinned staging ring (pool threads memcpy it
// into 16 MiB pinned slots that are DMA'd); SHELFI_H2D_DIRECT=1 copies it straight from the caller's
// pageable memory instead, which is faster only on blobs the runtime has already pinned: on fresh blobs
// (every aggregation round's uploads) the runtime pins their pages on each first copy.  16 x 64 cts of
// archives, input GB/s fresh malloc'd / fresh encrypt outputs / warm: ring 48.2 / 48.9 / 48.5
// (profiles/r05u/slot_size.json, 16 MiB), direct 18.7 / 34.4 / 53.7 (taper_palisade.json).  The sum's D2H lands
// in a pinned buffer that the AsyncDrain worker scatters into the output, so the uploading thread never
// stops to drain.  (Zero-copy uploads registered in place with hipHostRegister measured slower than
// the ring and were removed in round 5: tools/h2d_register_ab.py.)
static void wavg_bytes_pipeline(shelfi_ctx* ctx, const std::vector<CtLayout>& in,
                                const float* weights, size_t C, uint64_t K, const CtLayout& dst,
                                const size_t* lens) {
  const Params& p = ctx->p;
  const size_t ct_bytes = 2ull * p.L * p.N * 8;
  const bool direct = switches().h2d_direct;
  // learners per wavg launch: all of them, up to kWavgMaxLearners (more: accumulated groups).  Cutting a
  // single-chunk call (cfg2's 16 x 4 cts) into 2 / 4 / 8 groups to overlap uploads with the device work
  // measured the same as one group once a step's learners share the ring's slots (profiles/r05ct)
  const size_t group = std::min<size_t>(C, kWavgMaxLearners);
  // chunk of input per learner-group buffer: direct uploads want ~32 MiB per copy (8 MiB copies ran
  // 51.6 GB/s, 2 MiB 41.3, 32 MiB 55.6, on pinned-warm blobs), so 32 MiB per learner; through the ring
  // ~128 MiB per group (round 4: 32 / 64 / 128 / 256 MiB ran 60.4 / 52.4 / 48.2 / 48.7 ms for 16 learners x
  // 64 cts, profiles/r04w/api_chunk.txt); SHELFI_WAVG_CHUNK_MIB overrides (A/B probe switch)
  const uint64_t chunk_mib = switches().wavg_chunk_mib ? switches().wavg_chunk_mib : direct ? 32 * group : 128;
  uint64_t kc = std::max<uint64_t>(1, (chunk_mib << 20) / (ct_bytes * group));
  // at least ~4 chunks through the ring, so a small call's gather + wavg + D2H overlap its later uploads: cfg2's
  // 16 x 4 cts in 4 chunks ran 41.0 / 44.4 / 42.8 GB/s (fresh copies / fresh encrypt outputs / warm) vs 39.0 /
  // 41.8 / 40.5 in one (profiles/r05cy)
  if (!direct && !switches().wavg_chunk_mib) kc = std::min<uint64_t>(kc, std::max<uint64_t>(1, (K + 3) / 4));
  // packed wire (version-2 blobs): uploads land packed and are unpacked on the device; a packed
  // output is packed before its D2H
  // seeded inputs (version-3 blobs): each ciphertext's c0 lands as one packed group; it is unpacked into
  // polynomial 0 and c1 expanded beside it, both on the compute stream
  const bool sin = in.front().seeded;
  const uint64_t pct = 2 * packed_poly_bytes(p, p.L), pct_in = sin ? pct / 2 : pct;
  const bool pin = in.front().packed || sin, pout = dst.packed;
  const bool raw = in.front().pal;  // archives: raw ranges, gathered on the device
  kc = std::min<uint64_t>(kc, K);
  const size_t in_chunk = group * kc * ct_bytes, out_chunk = kc * ct_bytes;
  const size_t pin_chunk = pin ? group * kc * pct_in : 0, pout_chunk = pout ? kc * pct : 0;
  const uint64_t nchunks = (K + kc - 1) / kc;
  std::vector<HostPiece> pcs;
  // raw ranges: a step's (chunk, learner group) learners' byte ranges (tower headers included) land back to
  // back in its raw buffer, so the ring packs them into full slots (one DMA per slot, not per learner: each
  // DMA costs ~17 us of gap on the copy engine, profiles/r05cp); the whole call's gather table -- every
  // step's run offsets into its raw buffer -- is written once into pinned memory and uploaded by one copy
  // ahead of the data (no per-step table copies or host waits)
  size_t raw_cap = 0, runs_total = 0;  // raw_cap: the largest step's bytes
  std::vector<size_t> step_run0;       // step -> its first table entry
  if (raw) {
    for (uint64_t ci = 0; ci < nchunks; ++ci) {
      const uint64_t k0 = ci * kc, kn = std::min<uint64_t>(kc, K - k0);
      for (size_t c0 = 0; c0 < C; c0 += group) {
        size_t bytes = 0;
        for (size_t c = c0; c < std::min(C, c0 + group); ++c) {
          in[c].pieces(k0, kn, p, pcs);
          bytes += (size_t)(pcs.back().p + pcs.back().n - pcs.front().p);
          runs_total += pcs.size();
        }
        raw_cap = std::max(raw_cap, bytes);
      }
    }
    raw_cap = (raw_cap + 64 + 255) & ~(size_t)255;  // + the gather's read-ahead of one dword
    if (ctx->gather_cap < runs_total) {
      if (ctx->gather_host) SHELFI_HIP(hipHostFree(ctx->gather_host));
      ctx->gather_host = nullptr;
      ctx->gather_cap = 0;
      SHELFI_HIP(hipHostMalloc((void**)&ctx->gather_host, runs_total * 8, hipHostMallocDefault));
      ctx->gather_cap = runs_total;
    }
    size_t r = 0;
    for (uint64_t ci = 0; ci < nchunks; ++ci) {
      const uint64_t k0 = ci * kc, kn = std::min<uint64_t>(kc, K - k0);
      for (size_t c0 = 0; c0 < C; c0 += group) {
        step_run0.push_back(r);
        size_t off = 0;
        for (size_t c = c0; c < std::min(C, c0 + group); ++c) {
          in[c].pieces(k0, kn, p, pcs);
          const uint8_t* lo = pcs.front().p;
          for (const HostPiece& h : pcs) ctx->gather_host[r++] = (uint64_t)(off + (size_t)(h.p - lo));
          off += (size_t)(pcs.back().p + pcs.back().n - lo);
        }
      }
    }
    step_run0.push_back(r);
  }
  const size_t raw_chunk = raw ? raw_cap : 0, tab_bytes = (runs_total * 8 + 255) & ~(size_t)255;
  uint8_t* io = (uint8_t*)ensure(ctx->io, ctx->io_bytes,
                                 2 * (in_chunk + out_chunk + pin_chunk + pout_chunk + raw_chunk) + tab_bytes);
  uint8_t* inb[2] = {io, io + in_chunk};
  uint8_t* outb[2] = {io + 2 * in_chunk, io + 2 * in_chunk + out_chunk};
  uint8_t* const pbase = io + 2 * (in_chunk + out_chunk);
  uint8_t* pinb[2] = {pbase, pbase + pin_chunk};
  uint8_t* poutb[2] = {pbase + 2 * pin_chunk, pbase + 2 * pin_chunk + pout_chunk};
  uint8_t* const rbase = pbase + 2 * (pin_chunk + pout_chunk);
  uint8_t* rawb[2] = {rbase, rbase + raw_chunk};
  uint64_t* const tabd = (uint64_t*)(rbase + 2 * raw_chunk);
  const ArenaPack ap = arena_pack(p);
  // A: H2D of the learners' slices; B: wavg; C: staged D2H of the sum
  Pipe pp(ctx);
  StageRun sr(stager(ctx));
  if (!ctx->drain) ctx->drain = new AsyncDrain(default_copy_threads());
  const bool two = direct && switches().h2d_two && C > 1;
  if (two && !ctx->up2) {
    if (!ctx->stream4) SHELFI_HIP(hipStreamCreateWithFlags(&ctx->stream4, hipStreamNonBlocking));
    ctx->up2 = new AsyncUpload();
  }
  hipEvent_t up2_done[2] = {nullptr, nullptr};
  struct EvGuard {
    hipEvent_t* e;
    ~EvGuard() {
      for (int i = 0; i < 2; ++i)
        if (e[i]) (void)hipEventDestroy(e[i]);
    }
  } eg{up2_done};
  if (two)
    for (int i = 0; i < 2; ++i) SHELFI_HIP(hipEventCreateWithFlags(&up2_done[i], hipEventDisableTiming));
  struct UpGuard {  // on an error: the second thread's posted copies are issued and done before we unwind
    shelfi_ctx* c;
    bool armed;
    ~UpGuard() {
      if (!armed) return;
      try {
        c->up2->wait();
      } catch (...) {
      }
      (void)hipStreamSynchronize(c->stream4);
    }
  } ug{ctx, two};
  struct DrainGuard {  // on an error: the worker finishes what was posted before the streams go away
    AsyncDrain* d;
    bool armed;
    ~DrainGuard() {
      if (armed && d) try {
          d->finish();
        } catch (...) {
        }
    }
  } dg{ctx->drain, true};
  {  // the output's residue pages, first-touched on the drain worker during the uploads
    dst.pieces(0, K, p, pcs);
    const uint8_t* lo = pcs.front().p;
    ctx->drain->prefault(const_cast<uint8_t*>(lo), (size_t)(pcs.back().p + pcs.back().n - lo));
  }
  uint32_t* bad = ctx->dev_flag + 3;  // an upload residue >= q (the kernels assume canonical inputs)
  SHELFI_HIP(hipMemsetAsync(bad, 0, 4, pp.b));
  if (raw) SHELFI_HIP(hipMemcpyAsync(tabd, ctx->gather_host, runs_total * 8, hipMemcpyHostToDevice, pp.a));
  using clk = std::chrono::steady_clock;
  const bool trace = sr.s.trace();
  const auto t_start = clk::now();
  double t_up = 0.0;  // SHELFI_STAGE_TRACE: host seconds in the uploads
  // input buffers alternate by step (a learner group of a chunk), the sum's buffers by chunk
  uint64_t st = 0;
  std::vector<HostPiece> grp;  // a step's host pieces, in landing order
  for (uint64_t ci = 0; ci < nchunks; ++ci) {
    const int b = (int)(ci & 1);
    const uint64_t k0 = ci * kc, kn = std::min<uint64_t>(kc, K - k0);
    for (size_t c0 = 0; c0 < C; c0 += group) {
      const size_t gc = std::min(group, C - c0);
      const int bi = (int)(st & 1);
      if (st >= 2) {  // buffer free
        SHELFI_HIP(hipStreamWaitEvent(pp.a, pp.computed[bi], 0));
        if (two) SHELFI_HIP(hipStreamWaitEvent(ctx->stream4, pp.computed[bi], 0));
      }
      // where the uploads land: the learners' uint64 slots, or their packed staging (then unpacked), or
      // (archives) their raw ranges back to back, gathered below -- contiguous in every case, so through
      // the ring the whole group is one gather of pieces
      uint8_t* const land0 = raw ? rawb[bi] : pin ? pinb[bi] : inb[bi];
      size_t off = 0;
      grp.clear();
      for (size_t c = 0; c < gc; ++c) {
        in[c0 + c].pieces(k0, kn, p, pcs);
        const uint8_t* lo = pcs.front().p;
        const size_t span = (size_t)(pcs.back().p + pcs.back().n - lo);
        if (direct) {  // one pageable copy of the learner's whole range
          uint8_t* land = land0 + (raw ? off : c * kn * (pin ? pct_in : ct_bytes));
          const auto t0 = clk::now();
          if (two && (c & 1))  // every other learner from the second thread: two copies in flight
            ctx->up2->post(land, lo, span, ctx->stream4);
          else
            SHELFI_HIP(hipMemcpyAsync(land, lo, span, hipMemcpyHostToDevice, pp.a));
          if (trace) t_up += std::chrono::duration<double>(clk::now() - t0).count();
        } else if (raw) {
          grp.push_back(HostPiece{const_cast<uint8_t*>(lo), span});
        } else {
          grp.insert(grp.end(), pcs.begin(), pcs.end());
        }
        off += span;
      }
      if (!direct) {
        const auto t0 = clk::now();
        sr.s.h2dv(land0, grp.data(), grp.size(), pp.a);
        if (trace) t_up += std::chrono::duration<double>(clk::now() - t0).count();
      }
      if (two) {  // the second thread's copies of this chunk join stream A
        ctx->up2->wait();
        SHELFI_HIP(hipEventRecord(up2_done[bi], ctx->stream4));
        SHELFI_HIP(hipStreamWaitEvent(pp.a, up2_done[bi], 0));
      }
      SHELFI_HIP(hipEventRecord(pp.in_ready[bi], pp.a));
      SHELFI_HIP(hipStreamWaitEvent(pp.b, pp.in_ready[bi], 0));
      if (raw)
        launch_gather_runs(rawb[bi], tabd + step_run0[st], step_run0[st + 1] - step_run0[st], (uint32_t)(p.N * 8),
                           inb[bi], pp.b);
      if (pin)  // unpacked on the compute stream, so the upload stream moves on to the next chunk
        for (size_t c = 0; c < gc; ++c) {
          uint64_t* const ub = (uint64_t*)(inb[bi] + c * kn * ct_bytes);
          if (sin)
            seeded_land(ctx, in[c0 + c], pinb[bi] + c * kn * pct_in, k0, kn, p.L, ap, ub, pp.b);
          else
            launch_blob_unpack((const uint32_t*)(pinb[bi] + c * kn * pct), kn, p.L, p.logN, ap, ub, pp.b);
        }
      if (ci >= 2 && c0 == 0) SHELFI_HIP(hipStreamWaitEvent(pp.b, pp.out_free[b], 0));
      WavgArgs a;
      std::memset(&a, 0, sizeof(a));
      for (size_t c = 0; c < gc; ++c) a.ptrs[c] = (const uint64_t*)(inb[bi] + c * kn * ct_bytes);
      fill_weights(a, p, weights + c0, gc);
      a.out = (uint64_t*)outb[b];
      a.rows = kn * 2 * p.L;
      a.C = (uint32_t)gc;
      a.L = p.L;
      a.logN = p.logN;
      a.accumulate = c0 ? 1 : 0;
      a.bad = bad;
      launch_wavg(a, ctx->dt.tc, pp.b);
      SHELFI_HIP(hipEventRecord(pp.computed[bi], pp.b));
      ++st;
      if (c0 + gc >= C) {
        if (pout) {  // the sum is canonical: the residue check cannot fire
          launch_blob_pack((const uint64_t*)outb[b], kn, p.L, p.logN, ap, ctx->dt.tc, (uint32_t*)poutb[b],
                           ctx->dev_flag + 5, pp.b);
          SHELFI_HIP(hipEventRecord(pp.computed[bi], pp.b));
        }
        // the last chunk's D2H follows its wavg on the compute stream (nothing is left to overlap, and the
        // cross-stream event cost ~0.1 ms before it: profiles/r05cp)
        const hipStream_t ds = ci + 1 == nchunks ? pp.b : pp.c;
        if (ds == pp.c) SHELFI_HIP(hipStreamWaitEvent(pp.c, pp.computed[bi], 0));
        dst.pieces(k0, kn, p, pcs);
        const uint8_t* sum = pout ? poutb[b] : outb[b];
        // one DMA into the drain's pinned buffer; its worker scatters it to the pieces
        size_t nbytes = 0;
        for (const HostPiece& h : pcs) nbytes += h.n;
        uint8_t* hb = ctx->drain->buffer(b, nbytes);  // waits until chunk ci - 2 is drained
        SHELFI_HIP(hipMemcpyAsync(hb, sum, nbytes, hipMemcpyDeviceToHost, ds));
        SHELFI_HIP(hipEventRecord(pp.out_free[b], ds));
        ctx->drain->post(b, pp.out_free[b], pcs);
      }
    }
  }
  SHELFI_HIP(hipMemcpyAsync(ctx->host_flag + 3, bad, 4, hipMemcpyDeviceToHost, pp.b));  // pinned: no sync copy
  const auto t_issued = clk::now();
  ctx->drain->finish();
  sr.finish();
  pp.sync();
  if (trace)
    std::fprintf(stderr, "[wavg-bytes] %s%s chunks %llu x %llu cts, %llu learners per group: issue %.2f ms "
                 "(uploads %.2f), tail %.2f ms\n", direct ? "direct" : "ring", raw ? "+gather" : "",
                 (unsigned long long)nchunks, (unsigned long long)kc, (unsigned long long)group,
                 std::chrono::duration<double>(t_issued - t_start).count() * 1e3, t_up * 1e3,
                 std::chrono::duration<double>(clk::now() - t_issued).count() * 1e3);
  if (ctx->host_flag[3])  // read back on pp.b before the sync above
    throw Error{SHELFI_ERR_FORMAT, "ciphertext residue >= its tower modulus (malformed learner data)"};
}

// The allocating form of an `_into` entry point: a size query, a malloc'd buffer (shelfi_free), the
// call, and the buffer freed again on an error.
template <class Into>
static int into_malloc(uint8_t** out, size_t* out_len, Into into) {
  size_t total = 0;
  int rc = into(nullptr, 0, &total);
  if (rc) return rc;
  uint8_t* buf = (uint8_t*)std::malloc(total ? total : 1);
  if (!buf) {
    set_error("host out of memory");
    return SHELFI_ERR_DEVICE;
  }
  rc = into(buf, total, &total);
  if (rc) {
    std::free(buf);
    return rc;
  }
  *out = buf;
  *out_len = total;
  return SHELFI_OK;
}

}  // namespace shelfi

extern "C" {

int shelfi_encrypt_into(shelfi_ctx* ctx, const double* x, size_t n, uint8_t* out, size_t out_cap,
                        size_t* out_len) {
  if (!ctx || !out_len || (n && !x)) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    require_keys(ctx);
    if (ctx->wire == 3) require_own_secret(ctx);
    DeviceGuard g(ctx->device);
    const Params& p = ctx->p;
    const uint64_t K = (n + values_per_ct(p) - 1) / values_per_ct(p);  // ckks.cpp:65
    size_t total = 0;
    make_output(ctx, ctx->wire, K, 1, 0, p.delta, nullptr, &total);
    *out_len = total;
    if (!out) return;
    if (out_cap < total) throw Error{SHELFI_ERR_ARG, "output buffer too small"};
    advise_huge(out, total);
    // residues first (the parallel drains first-touch the fresh pages), framing after
    CtLayout dst = make_output(ctx, ctx->wire, K, 1, 0, p.delta, nullptr, &total);
    dst.base = out;
    if (K || dst.seeded) {
      uint32_t key[8];
      KeyWiper wipe(key);
      uint64_t g0;
      draw_key(ctx, K, key, &g0);
      if (dst.seeded) seeded_seed(key, g0, dst.seed);  // an empty batch carries a seed too
      if (K) encrypt_bytes_pipeline(ctx, x, n, K, dst, key, g0, false);
    }
    make_output(ctx, ctx->wire, K, 1, 0, p.delta, out, &total, dst.seed);
  });
}

int shelfi_encrypt(shelfi_ctx* ctx, const double* x, size_t n, uint8_t** out, size_t* out_len) {
  if (!ctx || !out || !out_len || (n && !x)) return SHELFI_ERR_ARG;
  *out = nullptr;
  return into_malloc(out, out_len, [&](uint8_t* buf, size_t cap, size_t* len) {
    return shelfi_encrypt_into(ctx, x, n, buf, cap, len);
  });
}

int shelfi_weighted_average_into(shelfi_ctx* ctx, const uint8_t* const* blobs, const size_t* lens,
                                 const float* weights, size_t C, uint8_t* out, size_t out_cap,
                                 size_t* out_len) {
  if (!ctx || !out_len || (C && (!blobs || !lens || !weights))) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    if (C == 0) {
      // ckks.cpp:270-309: with no learners the loop never runs and the empty
      // vector<Ciphertext> is serialized; here an empty batch in the ctx's wire format
      // (depth 2 / scale Delta^2: what a weighted average of fresh ciphertexts carries)
      const int fmt = ctx->wire == 3 ? 2 : ctx->wire;  // an aggregate is never seeded
      const double scale = ctx->p.delta * ctx->p.delta;
      size_t total = 0;
      make_output(ctx, fmt, 0, 2, 0, scale, nullptr, &total);
      *out_len = total;
      if (!out) return;
      if (out_cap < total) throw Error{SHELFI_ERR_ARG, "output buffer too small"};
      make_output(ctx, fmt, 0, 2, 0, scale, out, &total);
      return;
    }
    using clk = std::chrono::steady_clock;
    const auto t_in = clk::now();
    check_wavg_weights(weights, C, ctx->p.delta);
    DeviceGuard g(ctx->device);
    const std::vector<CtLayout> in = wavg_inputs(ctx, blobs, lens, C);
    const auto t_parsed = clk::now();
    const CtLayout& h0 = in.front();
    // a sum of seeded ciphertexts is not seeded: the answer to seeded inputs is packed
    const int ofmt = h0.seeded ? 2 : h0.fmt();
    // EvalMult by a constant (ckks.cpp:288): depth + 1, scale * Delta, same level
    const uint32_t depth = h0.depth + 1;
    const double scale = h0.scale * ctx->p.delta;
    size_t total = 0;
    make_output(ctx, ofmt, h0.K, depth, h0.level, scale, nullptr, &total);
    *out_len = total;
    if (!out) return;  // size query
    if (out_cap < total) throw Error{SHELFI_ERR_ARG, "output buffer too small"};
    advise_huge(out, total);
    // residues first (the parallel drains first-touch the fresh pages), framing after
    CtLayout dst = make_output(ctx, ofmt, h0.K, depth, h0.level, scale, nullptr, &total);
    dst.base = out;
    const auto t_pipe = clk::now();
    if (h0.K) wavg_bytes_pipeline(ctx, in, weights, C, h0.K, dst, lens);
    const auto t_done = clk::now();
    make_output(ctx, ofmt, h0.K, depth, h0.level, scale, out, &total);
    if (switches().stage_trace) {
      const auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count() * 1e3; };
      std::fprintf(stderr, "[wavg-call] parse %.3f ms, setup %.3f, pipeline %.3f, framing %.3f, total %.3f\n",
                   ms(t_in, t_parsed), ms(t_parsed, t_pipe), ms(t_pipe, t_done), ms(t_done, clk::now()),
                   ms(t_in, clk::now()));
    }
  });
}

int shelfi_weighted_average(shelfi_ctx* ctx, const uint8_t* const* blobs, const size_t* lens,
                            const float* weights, size_t C, uint8_t** out, size_t* out_len) {
  if (!ctx || !out || !out_len || (C && (!blobs || !lens || !weights))) return SHELFI_ERR_ARG;
  *out = nullptr;
  *out_len = 0;
  return into_malloc(out, out_len, [&](uint8_t* buf, size_t cap, size_t* len) {
    return shelfi_weighted_average_into(ctx, blobs, lens, weights, C, buf, cap, len);
  });
}

int shelfi_decrypt(shelfi_ctx* ctx, const uint8_t* blob, size_t len, size_t n, double* out) {
  if (!ctx || (n && !out)) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    require_keys(ctx);
    DeviceGuard g(ctx->device);
    const Params& p = ctx->p;
    require_no_flood_on_complex(ctx);
    const CtLayout h = open_cts(ctx, blob, len);
    if (n > h.K * values_per_ct(p))
      throw Error{SHELFI_ERR_ARG, "decrypt: data_dimensions exceeds the slots in the ciphertexts"};
    if (!n) return;
    // ckks.cpp:192-196: ciphertext i contributes min(batch, n - i*batch) values
    const uint64_t K = (n + values_per_ct(p) - 1) / values_per_ct(p);
    advise_huge(out, n * 8);
    const GenFlag fl = next_gen_flag(ctx);
    DecodeNoise dn = decode_noise_begin(ctx, K, fl);
    const uint64_t g0 = dn.g0;
    // one pipelined pass over the call: the decode's tower prefix (decode_towers: only those towers
    // are uploaded) with the fast CRT, or (exact) every tower through crt_exact_kernel
    const auto run = [&](bool exact) {
      const DecodePass pass = decode_pass(ctx, p.L, exact);
      const Params& pd = pass.p;
      const DeviceTables& dtd = pass.dt;
      const size_t ct_bytes = 2ull * pd.L * p.N * 8;  // only the decode's towers travel
      uint64_t kc = std::max<uint64_t>(1, (64ull << 20) / ct_bytes);
      kc = std::min<uint64_t>(kc, K);
      const size_t cin = kc * ct_bytes, dout = kc * values_per_ct(p) * 8;
      // a packed blob's tower prefix lands packed and is unpacked on the device
      // (a seeded blob's c0 prefix lands the same way, and c1's prefix is expanded beside it)
      const bool hp = h.packed || h.seeded;
      const uint64_t ppre = (h.seeded ? 1 : 2) * packed_poly_bytes(p, pd.L);  // packed bytes of one ciphertext's prefix
      const size_t pin = hp ? kc * ppre : 0;
      uint8_t* io = (uint8_t*)ensure(ctx->io, ctx->io_bytes, 2 * (cin + dout + pin));
      uint8_t* cb[2] = {io, io + cin};
      uint8_t* ob[2] = {io + 2 * cin, io + 2 * cin + dout};
      uint8_t* pb[2] = {io + 2 * (cin + dout), io + 2 * (cin + dout) + pin};
      const ArenaPack apd = arena_pack_prefix(p, pd.L);
      void* scratch = ensure(ctx->scratch, ctx->scratch_bytes, decrypt_scratch_bytes(pd, kc));
      Pipe pp(ctx);
      StageRun sr(stager(ctx));
      dn.g0 = g0;
      dn.reset = 1;
      std::vector<HostPiece> pcs;
      const uint64_t nchunks = (K + kc - 1) / kc;
      for (uint64_t ci = 0; ci < nchunks; ++ci) {
        const int b = (int)(ci & 1);
        const uint64_t k0 = ci * kc, kn = std::min<uint64_t>(kc, K - k0);
        const uint64_t o0 = k0 * values_per_ct(p), on = std::min<uint64_t>(n - o0, kn * values_per_ct(p));
        if (ci >= 2) SHELFI_HIP(hipStreamWaitEvent(pp.a, pp.computed[b], 0));
        h.pieces(k0, kn, p, pcs, pd.L);
        sr.s.h2dv(hp ? pb[b] : cb[b], pcs.data(), pcs.size(), pp.a);
        SHELFI_HIP(hipEventRecord(pp.in_ready[b], pp.a));
        SHELFI_HIP(hipStreamWaitEvent(pp.b, pp.in_ready[b], 0));
        if (h.packed) launch_blob_unpack((const uint32_t*)pb[b], kn, pd.L, p.logN, apd, (uint64_t*)cb[b], pp.b);
        if (h.seeded) seeded_land(ctx, h, pb[b], k0, kn, pd.L, apd, (uint64_t*)cb[b], pp.b);
        if (ci >= 2) SHELFI_HIP(hipStreamWaitEvent(pp.b, pp.out_free[b], 0));
        dn.g0 += (ci ? kc : 0);
        launch_decrypt(pd, dtd, ctx->dk, (const uint64_t*)cb[b], kn, h.scale, on, (double*)ob[b],
                       scratch, pp.b, &dn, false, 0, fl, exact);
        dn.reset = 0;
        SHELFI_HIP(hipEventRecord(pp.computed[b], pp.b));
        SHELFI_HIP(hipStreamWaitEvent(pp.c, pp.computed[b], 0));
        sr.s.d2h(out + o0, ob[b], on * 8, pp.c);
        SHELFI_HIP(hipEventRecord(pp.out_free[b], pp.c));
        sr.s.poll();
      }
      decode_noise_readback(ctx, dn);
      sr.finish();
      pp.sync();  // the pass has completed when run returns
    };
    decrypt_passes(ctx, fl, dn, run, [] {});
  });
}

// mkhe.cpp:395-400: this party's partial decryption of a ciphertext batch (any wire format), as an
// "SHPD" blob.  The batch is uploaded in chunks, partially decrypted on the device (threshold.hip) and
// copied out; free with shelfi_free.
int shelfi_partial_decrypt(shelfi_ctx* ctx, const uint8_t* blob, size_t len, int lead, uint8_t** out,
                           size_t* out_len) {
  if (!ctx || !out || !out_len) return SHELFI_ERR_ARG;
  *out = nullptr;
  *out_len = 0;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    require_keys(ctx);
    DeviceGuard g(ctx->device);
    const Params& p = ctx->p;
    const CtLayout h = open_cts(ctx, blob, len);
    const size_t poly_bytes = (size_t)p.L * p.N * 8;
    const size_t total = sizeof(BlobHeader) + h.K * poly_bytes;
    struct Free {
      uint8_t* p;
      ~Free() { std::free(p); }
    } res{(uint8_t*)std::malloc(total)};
    if (!res.p) throw std::bad_alloc();
    const BlobHeader hd = make_partial_header(ctx, h.K, h.depth, h.scale, lead != 0);
    std::memcpy(res.p, &hd, sizeof(hd));
    if (h.K) {
      const uint64_t kc = std::min<uint64_t>(h.K, std::max<uint64_t>(1, (64ull << 20) / (2 * poly_bytes)));
      const bool hp = h.packed || h.seeded;
      const uint64_t pct = (h.seeded ? 1 : 2) * packed_poly_bytes(p, p.L);
      const size_t cin = kc * 2 * poly_bytes, pout = kc * poly_bytes, pin = hp ? kc * pct : 0;
      uint8_t* io = (uint8_t*)ensure(ctx->io, ctx->io_bytes, cin + pout + pin);
      uint8_t *cb = io, *ob = io + cin, *pb = io + cin + pout;
      const ArenaPack ap = arena_pack(p);
      hipStream_t s = ctx->stream;
      StageRun sr(stager(ctx));
      std::vector<HostPiece> pcs;
      for (uint64_t k0 = 0; k0 < h.K; k0 += kc) {
        const uint64_t kn = std::min<uint64_t>(kc, h.K - k0);
        h.pieces(k0, kn, p, pcs);
        sr.s.h2dv(hp ? pb : cb, pcs.data(), pcs.size(), s);
        if (h.packed) launch_blob_unpack((const uint32_t*)pb, kn, p.L, p.logN, ap, (uint64_t*)cb, s);
        if (h.seeded) seeded_land(ctx, h, pb, k0, kn, p.L, ap, (uint64_t*)cb, s);
        partial_decrypt_locked(ctx, (const uint64_t*)cb, kn, p.L, lead != 0, (uint64_t*)ob, s);
        SHELFI_HIP(hipMemcpy(res.p + sizeof(BlobHeader) + k0 * poly_bytes, ob, kn * poly_bytes,
                             hipMemcpyDeviceToHost));
      }
      sr.finish();
    }
    *out = res.p;
    *out_len = total;
    res.p = nullptr;
  });
}

// mkhe.cpp:402 MultipartyDecryptFusion: P parties' "SHPD" partial decryptions of one ciphertext batch ->
// n doubles.  Needs no keys (the fusing party is the server); the scale comes from the headers.
int shelfi_fuse_decrypt(shelfi_ctx* ctx, const uint8_t* const* partials, const size_t* lens, size_t P, size_t n,
                        double* out) {
  if (!ctx || (n && !out)) return SHELFI_ERR_ARG;
  if (!partials || !lens || P < 1 || P > (size_t)kMaxCommRanks) {
    set_error("fuseDecrypt: 1..16 partial decryptions");
    return SHELFI_ERR_ARG;
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    const Params& p = ctx->p;
    require_no_flood_on_complex(ctx);
    std::vector<BlobHeader> hs(P);
    size_t leads = 0;
    for (size_t i = 0; i < P; ++i) {
      hs[i] = parse_partial(partials[i], lens[i], ctx);
      leads += hs[i].level;
      if (hs[i].key_id != hs[0].key_id || hs[i].K != hs[0].K || hs[i].depth != hs[0].depth ||
          hs[i].scale != hs[0].scale || hs[i].batch != hs[0].batch)
        throw Error{SHELFI_ERR_FORMAT, "fuseDecrypt: the partial decryptions do not belong to one ciphertext batch"};
    }
    if (leads != 1) throw Error{SHELFI_ERR_FORMAT, "fuseDecrypt: exactly one partial decryption must be the lead's"};
    if (hs[0].batch != p.batch) throw Error{SHELFI_ERR_FORMAT, "fuseDecrypt: batch size differs from the context's"};
    const uint64_t K = hs[0].K;
    if (n > K * values_per_ct(p))
      throw Error{SHELFI_ERR_ARG, "fuseDecrypt: data_dimensions exceeds the slots in the ciphertexts"};
    if (!n) return;
    DeviceGuard g(ctx->device);
    const uint64_t Kn = (n + values_per_ct(p) - 1) / values_per_ct(p);
    const size_t poly_bytes = (size_t)p.L * p.N * 8;
    const uint64_t kc = std::min<uint64_t>(Kn, std::max<uint64_t>(1, (64ull << 20) / (P * poly_bytes)));
    const size_t pin = kc * poly_bytes, dout = kc * values_per_ct(p) * 8;
    uint8_t* io = (uint8_t*)ensure(ctx->io, ctx->io_bytes, P * pin + dout);
    double* ob = (double*)(io + P * pin);
    hipStream_t s = ctx->stream;
    // the call's chunks each run the device driver: one redo and one logError (the maximum) per call
    const uint64_t redo0 = ctx->decode_redo_count;
    int log_error = -1;
    for (uint64_t k0 = 0; k0 < Kn; k0 += kc) {
      const uint64_t kn = std::min<uint64_t>(kc, Kn - k0);
      const uint64_t o0 = k0 * values_per_ct(p), on = std::min<uint64_t>(n - o0, kn * values_per_ct(p));
      FuseIn fz{};
      fz.P = (uint32_t)P;
      for (size_t i = 0; i < P; ++i) {
        SHELFI_HIP(hipMemcpyAsync(io + i * pin, partials[i] + sizeof(BlobHeader) + k0 * poly_bytes, kn * poly_bytes,
                                  hipMemcpyHostToDevice, s));
        fz.part[i] = (const uint64_t*)(io + i * pin);
      }
      dev_decrypt_locked(ctx, nullptr, kn, p.L, hs[0].scale, on, ob, s, false, &fz);
      SHELFI_HIP(hipMemcpy(out + o0, ob, on * 8, hipMemcpyDeviceToHost));
      if (ctx->log_error_pending && Kn > kc) {
        SHELFI_HIP(hipMemcpy(ctx->host_flag + 2, ctx->dev_flag + 2, 4, hipMemcpyDeviceToHost));
        log_error = std::max(log_error, (int)ctx->host_flag[2]);
        ctx->last_log_error = log_error;
        ctx->log_error_pending = false;
      }
    }
    if (ctx->decode_redo_count > redo0) ctx->decode_redo_count = redo0 + 1;
  });
}

}  // extern "C"
