// eval_keys.cpp — the evaluation keys' C ABI: EvalMultKeyGen and the
// rotation keys (mkhe.cpp:124, :274), get / set / save / load with PALISADE's key-eval-mult.txt, and the
// multiparty evaluation-key protocols of threshold CKKS (mkhe.cpp:271-317; multikey.hip).  The state the
// keys are installed into is eval_state.cpp; the operations that use them are in dev_api.cpp.
#include <algorithm>
#include <cstring>
#include <fstream>
#include <sstream>

#include "api_internal.h"
#include "eval_internal.h"
#include "palisade_codec.h"

namespace shelfi {

// key-eval-mult.txt metadata of this context's evaluation key (PALISADE keys required: the
// file embeds the context object and key tag of key-public.txt)
static PalisadeEvalKey evalkey_meta(const shelfi_ctx* ctx, const EvalState& ev) {
  if (ctx->pal_ctx_obj.empty() || ctx->pal_keytag.empty())
    throw Error{SHELFI_ERR_STATE, "evaluation-key files need PALISADE keys (loadCryptoParams or keygen)"};
  const Params& p = ctx->p;
  PalisadeEvalKey K;
  uint32_t id0 = 0;
  K.ctx = palisade_parse_context_object(ctx->pal_ctx_obj, &id0, 1);
  K.keytag = ctx->pal_keytag;
  K.N = p.N;
  K.T = p.L + ev.kP;
  K.dnum = ev.dnum;
  for (uint32_t t = 0; t < K.T; ++t) {
    K.q.push_back(t < p.L ? p.q[t] : ev.p[t - p.L]);
    K.psi.push_back(t < p.L ? p.psi[t] : ev.ppsi[t - p.L]);
  }
  // class versions as in the reference's own key-eval-mult.txt
  for (auto& v : K.poly_versions) v = 0;
  return K;
}

static std::string slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw Error{SHELFI_ERR_IO, "cannot read " + path};
  std::ostringstream ss;
  ss << f.rdbuf();
  return ss.str();
}

// install a parsed PALISADE evaluation key after checking it belongs to these keys / params
static void load_evalkey(shelfi_ctx* ctx, const std::string& file) {
  EvalState& ev = eval_state(ctx);
  const PalisadeEvalKey K = palisade_parse_evalmult_key((const uint8_t*)file.data(), file.size());
  const Params& p = ctx->p;
  if (ctx->pal_keytag.empty() || K.keytag != ctx->pal_keytag)
    throw Error{SHELFI_ERR_FORMAT, "evaluation key belongs to another key pair (key tag)"};
  if (K.N != p.N || K.T != p.L + ev.kP || K.dnum != ev.dnum)
    throw Error{SHELFI_ERR_FORMAT, "evaluation key was made for other parameters"};
  for (uint32_t t = 0; t < K.T; ++t)
    if (K.q[t] != (t < p.L ? p.q[t] : ev.p[t - p.L]))
      throw Error{SHELFI_ERR_FORMAT, "evaluation key towers differ from this context's Q and special primes"};
  if (K.tower_off.size() != 2ull * K.dnum * K.T) throw Error{SHELFI_ERR_FORMAT, "evaluation key tower count"};
  // residues: the key's roots may differ from ours for the special primes (PALISADE picks its
  // own); the EVALUATION order then differs, so only keys on the same roots are accepted
  for (uint32_t t = 0; t < K.T; ++t)
    if (K.psi[t] != (t < p.L ? p.psi[t] : ev.ppsi[t - p.L]))
      throw Error{SHELFI_ERR_FORMAT, "evaluation key roots of unity differ from this context's"};
  std::vector<uint64_t> polys(K.tower_off.size() * (size_t)K.N);
  for (size_t i = 0; i < K.tower_off.size(); ++i)
    std::memcpy(polys.data() + i * K.N, file.data() + K.tower_off[i], (size_t)K.N * 8);
  install_evk(ctx, ev, polys.data());
}

// shelfi_load: a key-eval-mult.txt beside PALISADE keys is loaded when it is theirs
void load_evalkey_if_present(shelfi_ctx* ctx, const std::string& dir) {
  std::string file;
  try {
    file = slurp(dir + "key-eval-mult.txt");
  } catch (const Error&) {
    return;  // optional file
  }
  try {
    load_evalkey(ctx, file);
  } catch (const Error&) {
    // another key pair's or another ring's key (e.g. palisade_pybind's resources): not ours
  }
}

}  // namespace shelfi

using namespace shelfi;

extern "C" {

int shelfi_special_primes(uint32_t ring_dim, uint32_t num_towers, const uint64_t* moduli, uint32_t* dnum,
                          uint32_t* alpha, uint32_t* num_special, uint64_t* special, uint64_t* special_roots) {
  if (!moduli || !dnum || !alpha || !num_special || !special || num_towers < 1 ||
      num_towers > (uint32_t)kMaxTowers || ring_dim < 2 || (ring_dim & (ring_dim - 1)))
    return SHELFI_ERR_ARG;
  return guarded([&] {
    uint64_t p[kMaxTowers], r[kMaxTowers];
    special_primes(ring_dim, num_towers, moduli, dnum, alpha, num_special, p, r);
    for (uint32_t i = 0; i < *num_special; ++i) {
      special[i] = p[i];
      if (special_roots) special_roots[i] = r[i];
    }
  });
}

int shelfi_eval_key_info(const shelfi_ctx* ctx, uint32_t* dnum, uint32_t* alpha, uint32_t* num_special,
                         uint64_t* special, int* has_key) {
  if (!ctx || !dnum || !alpha || !num_special) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    uint64_t p[kMaxTowers];
    special_primes(ctx->p.N, ctx->p.L, ctx->p.q, dnum, alpha, num_special, p, nullptr);
    if (special)
      for (uint32_t i = 0; i < *num_special; ++i) special[i] = p[i];
    if (has_key) *has_key = (ctx->ev && ctx->ev->evk) ? 1 : 0;
  });
}

size_t shelfi_eval_key_words(const shelfi_ctx* ctx) {
  if (!ctx) return 0;
  uint32_t dn, al, kP;
  uint64_t p[kMaxTowers];
  special_primes(ctx->p.N, ctx->p.L, ctx->p.q, &dn, &al, &kP, p, nullptr);
  return 2ull * dn * (ctx->p.L + kP) * ctx->p.N;
}

}  // extern "C"

namespace shelfi {

// What a call that makes a key in the evaluation key's layout starts from (ctx lock held, device set): the top
// level's tables, the kernels' constants and scratch, the key's words, and the call's stream key, wiped with it.
struct EvkGen {
  EvalState& ev;
  LevelState& l;
  const EvkGenConst gc;
  const size_t words;
  void* scratch;
  uint32_t key[8];
  KeyWiper wipe{key};
  explicit EvkGen(shelfi_ctx* ctx)
      : ev(eval_state(ctx)), l(level(ctx, ctx->p.L)), gc(evk_gen_const(ctx->p, ev)),
        words(2ull * ev.dnum * (ctx->p.L + ev.kP) * ctx->p.N),
        scratch(ensure(ctx->scratch, ctx->scratch_bytes, evk_scratch_bytes(ctx->p.L, ev.kP, ctx->p.N))) {
    stream_key(ctx, key);
  }
};

// A key-switching key s' -> s on the device, read back: galois = 0: s' = s^2 (EvalMultKeyGen);
// galois = g: s' = sigma_g(s) (a rotation key).  ctx lock held, device set.
static std::vector<uint64_t> switch_keygen(shelfi_ctx* ctx, uint32_t galois) {
  require_keys(ctx);
  EvkGen k(ctx);
  DevWords evk_d(k.words);
  std::vector<uint64_t> host(k.words);
  launch_evk_keygen(k.gc, ctx->dt, k.l.ext, ctx->dt.cdt, ctx->dt.cdt_len, k.key, ctx->dk.sk, evk_d.p, k.scratch,
                    ctx->stream, galois);
  SHELFI_HIP(hipMemcpyAsync(host.data(), evk_d.p, k.words * 8, hipMemcpyDeviceToHost, ctx->stream));
  SHELFI_HIP(hipStreamSynchronize(ctx->stream));
  return host;
}

static void rotation_keygen(shelfi_ctx* ctx, const int32_t* indices, size_t n) {
  require_keys(ctx);
  DeviceGuard dg(ctx->device);
  EvalState& ev = eval_state(ctx);
  std::vector<uint32_t> gs(n);
  size_t fresh = 0;  // refuse a list that would not fit before generating any of it
  for (size_t i = 0; i < n; ++i) {
    gs[i] = indices[i] ? rotation_galois(ctx, indices[i]) : 0;
    if (gs[i] && !find_rot(&ev, gs[i]) && std::find(gs.begin(), gs.begin() + i, gs[i]) == gs.begin() + i) ++fresh;
  }
  if (ev.rot.size() + fresh > kMaxRotKeys) throw Error{SHELFI_ERR_ARG, "a context holds at most 64 rotation keys"};
  for (size_t i = 0; i < n; ++i)
    if (gs[i]) install_rot(ctx, ev, indices[i], gs[i], switch_keygen(ctx, gs[i]).data());
}
}  // namespace shelfi

extern "C" {

int shelfi_eval_mult_keygen(shelfi_ctx* ctx) {
  if (!ctx) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    DeviceGuard g(ctx->device);
    const std::vector<uint64_t> host = switch_keygen(ctx, 0);
    install_evk(ctx, eval_state(ctx), host.data());
  });
}

int shelfi_galois_element(uint32_t ring_dim, int32_t index, uint32_t* g) {
  if (!g || ring_dim < 4 || ring_dim > (1u << 17) || (ring_dim & (ring_dim - 1)) ||
      index <= -(int64_t)(ring_dim / 2) || index >= (int64_t)(ring_dim / 2)) {
    set_error("galois element: ring_dim a power of two in 4..2^17, |index| < ring_dim / 2");
    return SHELFI_ERR_ARG;
  }
  *g = galois_element(ring_dim, index);
  return SHELFI_OK;
}

int shelfi_rotation_keygen(shelfi_ctx* ctx, const int32_t* indices, size_t n) {
  if (!ctx || (n && !indices)) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] { rotation_keygen(ctx, indices, n); });
}

int shelfi_eval_sum_keygen(shelfi_ctx* ctx) {
  if (!ctx) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    std::vector<int32_t> idx;
    for (uint32_t r = 1; r < ctx->p.batch; r <<= 1) idx.push_back((int32_t)r);
    rotation_keygen(ctx, idx.data(), idx.size());
  });
}

int shelfi_rotation_key_indices(const shelfi_ctx* ctx, int32_t* out, size_t cap, size_t* n) {
  if (!ctx || !n || (cap && !out)) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  *n = ctx->ev ? ctx->ev->rot.size() : 0;
  for (size_t i = 0; i < *n && i < cap; ++i) out[i] = ctx->ev->rot[i].index;
  return SHELFI_OK;
}

int shelfi_get_rotation_key(const shelfi_ctx* ctx, int32_t index, uint64_t* key) {
  if (!ctx || !key) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    const EvalState::RotKey& r = require_rot(const_cast<shelfi_ctx*>(ctx), index, rotation_galois(ctx, index));
    std::memcpy(key, r.host.data(), r.host.size() * 8);
  });
}

int shelfi_set_rotation_key(shelfi_ctx* ctx, int32_t index, const uint64_t* key) {
  if (!ctx || !key) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    if (!index) throw Error{SHELFI_ERR_ARG, "rotation index 0 has no key"};
    DeviceGuard g(ctx->device);
    install_rot(ctx, eval_state(ctx), index, rotation_galois(ctx, index), key);
  });
}

// ---- conjugation: the key of g = 2N - 1, a rotation key listed under index 0 ----
int shelfi_conjugate_keygen(shelfi_ctx* ctx) {
  if (!ctx) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    require_keys(ctx);
    DeviceGuard dg(ctx->device);
    EvalState& ev = eval_state(ctx);
    const uint32_t g = conjugation_galois(ctx->p.N);
    if (!find_rot(&ev, g) && ev.rot.size() >= kMaxRotKeys)
      throw Error{SHELFI_ERR_ARG, "a context holds at most 64 rotation keys"};
    install_rot(ctx, ev, 0, g, switch_keygen(ctx, g).data());
  });
}

int shelfi_get_conjugation_key(const shelfi_ctx* ctx, uint64_t* key) {
  if (!ctx || !key) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    const EvalState::RotKey* r = find_rot(ctx->ev, conjugation_galois(ctx->p.N));
    if (!r) throw Error{SHELFI_ERR_STATE, "no conjugation key: call conjugateKeyGen() first"};
    std::memcpy(key, r->host.data(), r->host.size() * 8);
  });
}

int shelfi_set_conjugation_key(shelfi_ctx* ctx, const uint64_t* key) {
  if (!ctx || !key) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    DeviceGuard g(ctx->device);
    install_rot(ctx, eval_state(ctx), 0, conjugation_galois(ctx->p.N), key);
  });
}

int shelfi_get_eval_key(const shelfi_ctx* ctx, uint64_t* evk) {
  if (!ctx || !evk) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);  // against a concurrent keygen / load replacing it
  if (!ctx->ev || ctx->ev->evk_host.empty()) {
    set_error("no evaluation key: call shelfi_eval_mult_keygen first");
    return SHELFI_ERR_STATE;
  }
  std::memcpy(evk, ctx->ev->evk_host.data(), ctx->ev->evk_host.size() * 8);
  return SHELFI_OK;
}

int shelfi_set_eval_key(shelfi_ctx* ctx, const uint64_t* evk) {
  if (!ctx || !evk) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    DeviceGuard g(ctx->device);
    install_evk(ctx, eval_state(ctx), evk);
  });
}

int shelfi_palisade_evalkey_parse(const uint8_t* file, size_t len, shelfi_palisade_evk_info* info,
                                  uint64_t* polys) {
  if (!file || !info) return SHELFI_ERR_ARG;
  return guarded([&] {
    const PalisadeEvalKey K = palisade_parse_evalmult_key(file, len);
    std::memset(info, 0, sizeof(*info));
    info->ring_dim = K.N;
    info->num_towers = K.T;
    info->ctx_towers = K.ctx.L;
    info->dnum = K.dnum;
    for (uint32_t t = 0; t < K.T; ++t) {
      info->moduli[t] = K.q[t];
      info->roots[t] = K.psi[t];
    }
    std::memcpy(info->keytag, K.keytag.data(), std::min<size_t>(K.keytag.size(), 256));
    if (polys)
      for (size_t i = 0; i < K.tower_off.size(); ++i)
        std::memcpy(polys + i * (size_t)K.N, file + K.tower_off[i], (size_t)K.N * 8);
  });
}

int shelfi_palisade_evalkey_rewrite(const uint8_t* file, size_t len, const uint64_t* polys, uint8_t** out,
                                    size_t* out_len) {
  if (!file || !polys || !out || !out_len) return SHELFI_ERR_ARG;
  *out = nullptr;
  *out_len = 0;
  return guarded([&] {
    const PalisadeEvalKey K = palisade_parse_evalmult_key(file, len);
    const std::string w = palisade_evalmult_key_file(K, polys);
    uint8_t* buf = (uint8_t*)std::malloc(w.size());
    if (!buf) throw std::bad_alloc();
    std::memcpy(buf, w.data(), w.size());
    *out = buf;
    *out_len = w.size();
  });
}

int shelfi_save_eval_key(const shelfi_ctx* ctx, const char* path) {
  if (!ctx || !path) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    if (!ctx->ev || ctx->ev->evk_host.empty())
      throw Error{SHELFI_ERR_STATE, "no evaluation key: call evalMultKeyGen() first"};
    const std::string w = palisade_evalmult_key_file(evalkey_meta(ctx, *ctx->ev), ctx->ev->evk_host.data());
    std::ofstream f(path, std::ios::binary);
    if (!f || !f.write(w.data(), (std::streamsize)w.size()))
      throw Error{SHELFI_ERR_IO, std::string("cannot write ") + path};
  });
}

int shelfi_load_eval_key(shelfi_ctx* ctx, const char* path) {
  if (!ctx || !path) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    DeviceGuard g(ctx->device);
    load_evalkey(ctx, slurp(path));
  });
}

}  // extern "C"

// ---- multiparty evaluation keys (mkhe.cpp:271-317; multikey.hip) ----
namespace shelfi {
namespace {
// the calls' device flag (dev_flag[7]): zeroed on the stream before the kernels, read back with the
// result before the call's one synchronisation
uint32_t* mk_flag_reset(shelfi_ctx* ctx) {
  uint32_t* flag = ctx->dev_flag + 7;
  SHELFI_HIP(hipMemsetAsync(flag, 0, 4, ctx->stream));
  return flag;
}

// result and flag back, one synchronisation; a raised flag refuses the call and leaves `out` untouched
void mk_finish(shelfi_ctx* ctx, const uint64_t* out_dev, size_t words, uint64_t* out) {
  std::vector<uint64_t> host(words);
  SHELFI_HIP(hipMemcpyAsync(ctx->host_flag + 7, ctx->dev_flag + 7, 4, hipMemcpyDeviceToHost, ctx->stream));
  SHELFI_HIP(hipMemcpyAsync(host.data(), out_dev, words * 8, hipMemcpyDeviceToHost, ctx->stream));
  SHELFI_HIP(hipStreamSynchronize(ctx->stream));
  const uint32_t f = ctx->host_flag[7];
  if (f & kMkBadResidue) throw Error{SHELFI_ERR_ARG, "multiparty key: a residue is >= its tower's modulus"};
  if (f & kMkADiffers)
    throw Error{SHELFI_ERR_ARG, "multiparty key: the keys' a-vectors differ (shares of different lead keys)"};
  std::memcpy(out, host.data(), words * 8);
}
}  // namespace
}  // namespace shelfi

extern "C" {

int shelfi_multi_key_switch_gen(shelfi_ctx* ctx, int32_t index, const uint64_t* prev, uint64_t* out) {
  if (!ctx || !out) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    require_keys(ctx);
    DeviceGuard dg(ctx->device);
    const uint32_t galois = index ? rotation_galois(ctx, index) : 1;  // 1: s' = s, the EvalMult share
    EvkGen k(ctx);
    DevWords out_d(k.words), prev_d(prev ? k.words : 0);
    if (prev) SHELFI_HIP(hipMemcpyAsync(prev_d.p, prev, k.words * 8, hipMemcpyHostToDevice, ctx->stream));
    uint32_t* flag = mk_flag_reset(ctx);
    launch_mk_share(k.gc, ctx->dt, k.l.ext, ctx->dt.cdt, ctx->dt.cdt_len, k.key, ctx->dk.sk, galois,
                    prev ? prev_d.p : nullptr, out_d.p, k.scratch, flag, ctx->stream);
    mk_finish(ctx, out_d.p, k.words, out);
  });
}

int shelfi_multi_add_eval_keys(shelfi_ctx* ctx, const uint64_t* const* keys, size_t n, int sum_a, uint64_t* out) {
  if (!ctx || !out || !keys) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    if (n < 1 || n > (size_t)kMkMaxKeys) throw Error{SHELFI_ERR_ARG, "multiparty key add takes 1..16 keys"};
    for (size_t i = 0; i < n; ++i)
      if (!keys[i]) throw Error{SHELFI_ERR_ARG, "multiparty key add: null key"};
    DeviceGuard dg(ctx->device);
    const Params& p = ctx->p;
    EvalState& ev = eval_state(ctx);
    LevelState& l = level(ctx, p.L);
    const EvkGenConst gc = evk_gen_const(p, ev);
    const size_t words = 2ull * ev.dnum * (p.L + ev.kP) * p.N;
    DevWords in_d(words * n), out_d(words);
    MkKeys mk{};
    mk.n = (uint32_t)n;
    for (size_t i = 0; i < n; ++i) {
      mk.k[i] = in_d.p + i * words;
      SHELFI_HIP(hipMemcpyAsync(in_d.p + i * words, keys[i], words * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    uint32_t* flag = mk_flag_reset(ctx);
    launch_mk_key_add(mk, gc, l.ext.tc, sum_a != 0, flag, out_d.p, ctx->stream);
    mk_finish(ctx, out_d.p, words, out);
  });
}

int shelfi_multi_mult_eval_key(shelfi_ctx* ctx, const uint64_t* joint, uint64_t* out) {
  if (!ctx || !out || !joint) return SHELFI_ERR_ARG;
  std::lock_guard<std::mutex> lk(ctx->mu);
  return guarded([&] {
    require_keys(ctx);
    DeviceGuard dg(ctx->device);
    EvkGen k(ctx);
    DevWords joint_d(k.words), out_d(k.words);
    SHELFI_HIP(hipMemcpyAsync(joint_d.p, joint, k.words * 8, hipMemcpyHostToDevice, ctx->stream));
    uint32_t* flag = mk_flag_reset(ctx);
    launch_mk_round2(k.gc, ctx->dt, k.l.ext, ctx->dt.cdt, ctx->dt.cdt_len, k.key, ctx->dk.sk, joint_d.p, out_d.p,
                     k.scratch, flag, ctx->stream);
    mk_finish(ctx, out_d.p, k.words, out);
  });
}

}  // extern "C"
