// eval_internal.h — the per-context evaluation state (eval_state.cpp) as the sources that use it see it: key
// generation and key I/O (eval_keys.cpp), the device operations (dev_api.cpp), decrypt at a level (call_state.cpp).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "shelfi_internal.h"

// Nothing declared here is part of libshelfi.so's dynamic symbol table.
#pragma GCC visibility push(hidden)

namespace shelfi {

constexpr int kMaxDigits = 3;  // ComputeNumLargeDigits never exceeds 3
constexpr size_t kMaxRotKeys = 64;

struct LevelState {
  bool built = false;  // key-switching state (ext, dtf, ks, args)
  bool q_built = false;
  bool own_q = false;  // q tables built here (levels below L); level L uses ctx->dt
  DeviceTables q;      // Q_l: NTT + CRT tables (decrypt at this level)
  DeviceTables ext;    // Q_l u P (key switching)
  DeviceTables dtf[kMaxDigits];  // per digit: its foreign towers (Q_l minus the digit, then P)
  uint64_t* ks = nullptr;
  KsArgs args{};
};

struct EvalState {
  uint32_t dnum = 0, alpha = 0, kP = 0;
  uint64_t p[kMaxTowers] = {0}, ppsi[kMaxTowers] = {0};
  std::string ks_error;        // why this chain cannot key-switch ("" = it can)
  uint64_t* evk = nullptr;     // [2][dnum][L + kP][N] (b-vector, a-vector)
  uint64_t* evk_sh = nullptr;  // Shoup companions
  std::vector<uint64_t> evk_host;
  // rotation keys sigma_g(s) -> s in the evaluation key's layout, keyed by the Galois element g
  struct RotKey {
    uint32_t g = 0;
    int32_t index = 0;  // the index it was first asked for under
    uint64_t* key = nullptr;
    uint64_t* key_sh = nullptr;
    std::vector<uint64_t> host;
  };
  std::vector<RotKey> rot;
  LevelState lv[kMaxTowers + 1];  // index = towers Ll
};

// Per-context level state, created on first use.  The special primes are derived here, but a chain that
// cannot key-switch (L + kP > 16) only fails EvalMult: decrypt and ModReduce at any level need nothing
// but the Q_l tables.
EvalState& eval_state(shelfi_ctx* ctx);
// NTT + CRT tables of Q_l = q_0 .. q_{Ll-1} (decrypt at a level, decode_pass): built on first use, no
// key-switching state.
const DeviceTables& level_q(shelfi_ctx* ctx, uint32_t Ll);
// Tables and key-switching constants for ciphertexts of Ll towers (Q_l = q_0 .. q_{Ll-1}).
LevelState& level(shelfi_ctx* ctx, uint32_t Ll);
// the constants of a key-generating kernel (keygen of s' -> s, the multiparty protocols)
EvkGenConst evk_gen_const(const Params& p, const EvalState& ev);

// g = 5^index mod 2N, the inverse for a negative index (PALISADE's FindAutomorphismIndex2nComplex)
uint32_t galois_element(uint32_t N, int32_t index);
// the same for a slot rotation of this context; |index| must be below the batch size
uint32_t rotation_galois(const shelfi_ctx* ctx, int32_t index);
// conjugation's: X -> X^(2N - 1) = X^-1 (below 2^18, the width of the key stream's g field)
inline uint32_t conjugation_galois(uint32_t N) { return 2u * N - 1u; }
EvalState::RotKey* find_rot(EvalState* ev, uint32_t g);
const EvalState::RotKey& require_rot(shelfi_ctx* ctx, int32_t index, uint32_t g);

// Install a key in the evaluation key's layout [2][dnum][L + kP][N] (host words; a residue >= its modulus
// is refused): the relinearization key, or the rotation key of Galois element g.
void install_evk(shelfi_ctx* ctx, EvalState& ev, const uint64_t* evk);
void install_rot(shelfi_ctx* ctx, EvalState& ev, int32_t index, uint32_t g, const uint64_t* key);

}  // namespace shelfi

#pragma GCC visibility pop
