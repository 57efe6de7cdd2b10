// eval_state.cpp — the per-context state of the general-circuit part of the PALISADE 1.11 CKKS scheme (SURVEY §8
// f4): the special primes, the per-level tables and HYBRID key-switching constants that EvalMult,
// ModReduce, the rotations (and decrypt at a level) use, and the installed relinearization and rotation keys.
// None of this is on the reference's aggregation path (ckks.cpp:26 fixes multDepth = 1, computeWeightedAverage
// only multiplies by constants).  Host code only precomputes constants and moves keys; every per-ciphertext step
// is in keyswitch.hip and rotate.hip.
#include <algorithm>

#include "api_internal.h"
#include "eval_internal.h"

namespace shelfi {

static uint64_t mm(uint64_t a, uint64_t b, uint64_t q) { return (uint64_t)(((u128)a * b) % q); }

// key-switching state of a level (its Q_l tables stay: decrypt at the level uses them)
static void free_level_ks(LevelState& l) {
  free_ntt_tables(l.ext);
  for (auto& d : l.dtf) free_ntt_tables(d);
  dfree_t(l.ks);
  l.ext = DeviceTables{};
  for (auto& d : l.dtf) d = DeviceTables{};
  l.args = KsArgs{};
  l.built = false;
}

static void free_level(LevelState& l) {
  if (l.own_q) free_ntt_tables(l.q);
  free_level_ks(l);
  l = LevelState{};
}

void eval_release(shelfi_ctx* ctx, bool keys_only) {
  EvalState* ev = ctx->ev;
  if (!ev) return;
  dfree_t(ev->evk);
  dfree_t(ev->evk_sh);
  ev->evk_host.clear();
  for (auto& r : ev->rot) {  // rotation keys belong to the secret key too
    dfree_t(r.key);
    dfree_t(r.key_sh);
  }
  ev->rot.clear();
  if (keys_only) return;
  for (auto& l : ev->lv) free_level(l);
  delete ev;
  ctx->ev = nullptr;
}

EvalState& eval_state(shelfi_ctx* ctx) {
  if (ctx->ev) return *ctx->ev;
  const Params& p = ctx->p;
  auto ev = new EvalState();
  try {
    special_primes(p.N, p.L, p.q, &ev->dnum, &ev->alpha, &ev->kP, ev->p, ev->ppsi);
    if (p.L + ev->kP > (uint32_t)kMaxTowers) ev->ks_error = "EvalMult needs num_towers + special primes <= 16";
  } catch (const Error& e) {
    ev->ks_error = e.msg;
  }
  ctx->ev = ev;
  return *ev;
}

const DeviceTables& level_q(shelfi_ctx* ctx, uint32_t Ll) {
  EvalState& ev = eval_state(ctx);
  const Params& P0 = ctx->p;
  require_towers(P0, Ll);
  LevelState& l = ev.lv[Ll];
  if (l.q_built) return l.q;
  if (Ll == P0.L) {
    l.q = ctx->dt;
    l.own_q = false;
  } else {
    Params pl = P0;
    pl.L = Ll;
    DeviceTables q;
    try {
      build_ntt_tables(pl, q);
    } catch (...) {
      free_ntt_tables(q);
      throw;
    }
    l.q = q;
    l.own_q = true;
    l.q.fft_inv = ctx->dt.fft_inv;  // shared, owned by the context
    l.q.fft_fwd = ctx->dt.fft_fwd;
    l.q.cdt = ctx->dt.cdt;
    l.q.cdt_len = ctx->dt.cdt_len;
  }
  l.q_built = true;
  return l.q;
}

LevelState& level(shelfi_ctx* ctx, uint32_t Ll) {
  EvalState& ev = eval_state(ctx);
  if (!ev.ks_error.empty()) throw Error{SHELFI_ERR_ARG, ev.ks_error};
  const Params& P0 = ctx->p;
  level_q(ctx, Ll);
  LevelState& l = ev.lv[Ll];
  if (l.built) return l;
  const uint32_t kP = ev.kP, T = Ll + kP, al = ev.alpha, dn = (Ll + al - 1) / al;
  try {
    Params pe = P0;
    pe.L = T;
    for (uint32_t m = 0; m < kP; ++m) {
      pe.q[Ll + m] = ev.p[m];
      pe.psi[Ll + m] = ev.ppsi[m];
    }
    build_ntt_tables(pe, l.ext);
    if (dn > (uint32_t)kMaxDigits) throw Error{SHELFI_ERR_ARG, "EvalMult: more than 3 digits"};
    for (uint32_t j = 0; j < dn; ++j) {  // digit j's foreign towers, in ModUp's order
      const uint32_t s = j * al, cnt = std::min(al, Ll - s);
      Params pf = P0;
      pf.L = T - cnt;
      for (uint32_t t = 0, u = 0; t < T; ++t)
        if (t < s || t >= s + cnt) {
          pf.q[u] = pe.q[t];
          pf.psi[u] = pe.psi[t];
          ++u;
        }
      build_ntt_tables(pf, l.dtf[j]);
    }
    // constants: mu_inv | mu_inv_sh [dn][al] | mu_hat [dn][al][T] | md_inv | md_inv_sh [kP] |
    // md_hat [kP][Ll] | pinv | pinv_sh [Ll]
    const size_t o_mi = 0, o_mis = o_mi + dn * al, o_mh = o_mis + dn * al, o_di = o_mh + (size_t)dn * al * T,
                 o_dis = o_di + kP, o_dh = o_dis + kP, o_pi = o_dh + (size_t)kP * Ll, o_pis = o_pi + Ll,
                 total = o_pis + Ll;
    std::vector<uint64_t> c(total, 0);
    for (uint32_t j = 0; j < dn; ++j) {
      const uint32_t s = j * al, cnt = std::min(al, Ll - s);
      for (uint32_t i = 0; i < cnt; ++i) {
        const uint64_t qi = pe.q[s + i];
        uint64_t h = 1;
        for (uint32_t u = 0; u < cnt; ++u)
          if (u != i) h = mm(h, pe.q[s + u] % qi, qi);
        const uint64_t inv = invmod(h, qi);
        c[o_mi + j * al + i] = inv;
        c[o_mis + j * al + i] = shoup(inv, qi);
        for (uint32_t t = 0; t < T; ++t) {
          const uint64_t qt = pe.q[t];
          uint64_t v = 1;
          for (uint32_t u = 0; u < cnt; ++u)
            if (u != i) v = mm(v, pe.q[s + u] % qt, qt);
          c[o_mh + ((size_t)j * al + i) * T + t] = v;
        }
      }
    }
    for (uint32_t m = 0; m < kP; ++m) {
      const uint64_t pm = ev.p[m];
      uint64_t h = 1;
      for (uint32_t u = 0; u < kP; ++u)
        if (u != m) h = mm(h, ev.p[u] % pm, pm);
      const uint64_t inv = invmod(h, pm);
      c[o_di + m] = inv;
      c[o_dis + m] = shoup(inv, pm);
      for (uint32_t t = 0; t < Ll; ++t) {
        const uint64_t qt = P0.q[t];
        uint64_t v = 1;
        for (uint32_t u = 0; u < kP; ++u)
          if (u != m) v = mm(v, ev.p[u] % qt, qt);
        c[o_dh + (size_t)m * Ll + t] = v;
      }
    }
    for (uint32_t t = 0; t < Ll; ++t) {
      const uint64_t qt = P0.q[t];
      uint64_t pm = 1;
      for (uint32_t u = 0; u < kP; ++u) pm = mm(pm, ev.p[u] % qt, qt);
      const uint64_t inv = invmod(pm, qt);
      c[o_pi + t] = inv;
      c[o_pis + t] = shoup(inv, qt);
    }
    l.ks = upload(c.data(), total);
    KsArgs& a = l.args;
    a.Ll = Ll;
    a.kP = kP;
    a.T = T;
    a.dn = dn;
    a.alpha = al;
    a.logN = P0.logN;
    a.Lfull = P0.L;
    a.dnFull = ev.dnum;
    a.mu_inv = l.ks + o_mi;
    a.mu_inv_sh = l.ks + o_mis;
    a.mu_hat = l.ks + o_mh;
    a.md_inv = l.ks + o_di;
    a.md_inv_sh = l.ks + o_dis;
    a.md_hat = l.ks + o_dh;
    a.pinv = l.ks + o_pi;
    a.pinv_sh = l.ks + o_pis;
    a.tq = ctx->dt.tc;  // q / Shoup constants only: the context's prefix serves every level
    a.te = l.ext.tc;
  } catch (...) {
    free_level_ks(l);
    throw;
  }
  l.built = true;
  return l;
}

// Shoup companions of a key in the evaluation key's layout, [2][dnum][L + kP][N]; a residue >= its
// modulus is refused (`what` names the key)
static std::vector<uint64_t> key_shoup(shelfi_ctx* ctx, EvalState& ev, const uint64_t* evk, const char* what) {
  const Params& p = ctx->p;
  if (!ev.ks_error.empty()) throw Error{SHELFI_ERR_ARG, ev.ks_error};
  const uint32_t T0 = p.L + ev.kP;
  const size_t TN = (size_t)T0 * p.N, words = 2ull * ev.dnum * TN;
  std::vector<uint64_t> sh(words);
  for (size_t i = 0; i < words; ++i) {
    const uint32_t t = (uint32_t)((i % TN) / p.N);
    const uint64_t q = t < p.L ? p.q[t] : ev.p[t - p.L];
    if (evk[i] >= q) throw Error{SHELFI_ERR_FORMAT, std::string(what) + " residue >= modulus"};
    sh[i] = shoup(evk[i], q);
  }
  return sh;
}

void install_evk(shelfi_ctx* ctx, EvalState& ev, const uint64_t* evk) {
  const std::vector<uint64_t> sh = key_shoup(ctx, ev, evk, "evaluation key");
  const size_t words = sh.size();
  dfree_t(ev.evk);
  dfree_t(ev.evk_sh);
  ev.evk_host.assign(evk, evk + words);
  ev.evk = upload(evk, words);
  ev.evk_sh = upload(sh.data(), words);
}

uint32_t galois_element(uint32_t N, int32_t index) {
  const uint64_t M = 2ull * N;
  const uint64_t n = index < 0 ? (uint64_t)(-(int64_t)index) : (uint64_t)index;
  uint64_t g = 1;
  for (uint64_t i = 0; i < n; ++i) g = g * 5 % M;
  if (index < 0) {  // g^-1 mod 2^k = g^(2^(k-2) - 1): the odd residues' exponent divides N / 2
    uint64_t inv = 1, b = g;
    for (uint64_t e = N / 2 - 1; e; e >>= 1, b = b * b % M)
      if (e & 1) inv = inv * b % M;
    g = inv;
  }
  return (uint32_t)g;
}

uint32_t rotation_galois(const shelfi_ctx* ctx, int32_t index) {
  const int64_t batch = ctx->p.batch;
  if (index <= -batch || index >= batch) throw Error{SHELFI_ERR_ARG, "rotation index must be below the batch size"};
  return galois_element(ctx->p.N, index);
}

EvalState::RotKey* find_rot(EvalState* ev, uint32_t g) {
  if (ev)
    for (auto& r : ev->rot)
      if (r.g == g) return &r;
  return nullptr;
}

const EvalState::RotKey& require_rot(shelfi_ctx* ctx, int32_t index, uint32_t g) {
  const EvalState::RotKey* r = find_rot(ctx->ev, g);
  if (!r)
    throw Error{SHELFI_ERR_STATE, "no rotation key for index " + std::to_string(index) +
                                      ": call rotationKeyGen() / evalSumKeyGen() first"};
  return *r;
}

void install_rot(shelfi_ctx* ctx, EvalState& ev, int32_t index, uint32_t g, const uint64_t* key) {
  const std::vector<uint64_t> sh = key_shoup(ctx, ev, key, "rotation key");
  const size_t words = sh.size();
  EvalState::RotKey* r = find_rot(&ev, g);
  if (!r) {
    if (ev.rot.size() >= kMaxRotKeys) throw Error{SHELFI_ERR_ARG, "a context holds at most 64 rotation keys"};
    ev.rot.emplace_back();
    r = &ev.rot.back();
    r->g = g;
    r->index = index;
  }
  uint64_t *kd = nullptr, *ks = nullptr;
  try {
    kd = upload(key, words);
    ks = upload(sh.data(), words);
  } catch (...) {
    dfree_t(kd);
    if (!r->key) ev.rot.pop_back();  // a new entry that never got its key
    throw;
  }
  dfree_t(r->key);
  dfree_t(r->key_sh);
  r->key = kd;
  r->key_sh = ks;
  r->host.assign(key, key + words);
}

EvkGenConst evk_gen_const(const Params& p, const EvalState& ev) {
  EvkGenConst gc{};
  gc.q0 = p.q[0];
  for (uint32_t t = 0; t < p.L; ++t) {
    gc.pmod[t] = 1;
    for (uint32_t m = 0; m < ev.kP; ++m) gc.pmod[t] = mm(gc.pmod[t], ev.p[m] % p.q[t], p.q[t]);
  }
  gc.L = p.L;
  gc.kP = ev.kP;
  gc.dnum = ev.dnum;
  gc.alpha = ev.alpha;
  gc.logN = p.logN;
  return gc;
}

}  // namespace shelfi
