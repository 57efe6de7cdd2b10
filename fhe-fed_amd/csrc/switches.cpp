// switches.cpp — the process-wide A/B probe switches (shelfi_internal.h Switches): the only reader of the
// SHELFI_* environment variables among the C-ABI sources.
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "shelfi_internal.h"

namespace shelfi {

// Process-wide switches: each reload publishes a new immutable snapshot through an
// atomic pointer; snapshots are never freed (a few dozen bytes per reload), so a launch path on
// another thread reads a consistent struct, never one being written.
static std::atomic<const Switches*> g_switches{nullptr};

static bool env_flag(const char* name, char off_or_on, bool dflt) {
  const char* e = getenv(name);
  return e && *e == off_or_on ? !dflt : dflt;
}
static int env_choice(const char* name, std::initializer_list<int> allowed, int dflt) {
  const char* e = getenv(name);
  if (!e) return dflt;
  const int v = atoi(e);
  for (int a : allowed)
    if (a == v) return v;
  return dflt;
}

void reload_switches() {
  Switches s;
  s.xcd_order = env_flag("SHELFI_XCD_ORDER", '0', true);
  s.ntt_wl = env_flag("SHELFI_NTT_WL", '0', true);
  s.fft_ct = env_flag("SHELFI_FFT_CT", '0', true);
  s.fft_whole = env_flag("SHELFI_FFT_WHOLE", '0', true);
  s.enc_fused = env_flag("SHELFI_ENC_FUSED_COLS", '0', true);
  s.enc_pp = env_flag("SHELFI_ENC_PP", '0', true);
  s.dec_pp = env_flag("SHELFI_DEC_PP", '0', true);
  s.enc_nored = env_flag("SHELFI_ENC_NORED", '0', true);
  s.enc_tab = env_flag("SHELFI_ENC_TAB", '0', true);
  s.enc_vt = env_flag("SHELFI_ENC_VT", '0', true);
  s.enc_ts = env_choice("SHELFI_ENC_TS", {0, 1}, -1);
  s.dec_all_towers = env_flag("SHELFI_DEC_ALL_TOWERS", '1', false);
  s.enc_x5 = env_flag("SHELFI_ENC_X5", '0', true);
  s.stage_trace = env_choice("SHELFI_STAGE_TRACE", {0, 1}, 0) == 1;
  if (const char* e = getenv("SHELFI_PACK_KERNEL")) s.pack_kernel = !strcmp(e, "v4") ? 4 : !strcmp(e, "r3") ? 3 : 0;
  s.pack_unroll = env_choice("SHELFI_PACK_UNROLL", {1, 2, 4, 8}, 0);
  s.pack_waves = env_choice("SHELFI_PACK_WAVES", {2, 8}, 0);
  s.wavg_rows = env_choice("SHELFI_WAVG_ROWS", {1, 2}, 0);
  if (const char* e = getenv("SHELFI_WAVG_STRANDS"))
    if (atoi(e) > 1 && atoi(e) <= 4096) s.wavg_strands = (uint32_t)atoi(e);
  s.arena_stager = env_choice("SHELFI_ARENA_STAGER", {0, 1}, -1);
  if (const char* e = getenv("SHELFI_DEV_CHUNK_MIB"))
    if (atoll(e) > 0) s.dev_chunk_mib = (uint64_t)atoll(e);
  if (const char* e = getenv("SHELFI_EVAL_CHUNK_MIB"))
    if (atoll(e) > 0) s.eval_chunk_mib = (uint64_t)atoll(e);
  if (const char* e = getenv("SHELFI_DOT_SLICE_CTS"))
    if (atoll(e) > 0) s.dot_slice_cts = (uint64_t)atoll(e);
  if (const char* e = getenv("SHELFI_GRAM_SLICE_CTS"))
    if (atoll(e) > 0) s.gram_slice_cts = (uint64_t)atoll(e);
  if (const char* e = getenv("SHELFI_DOTP_SLICE_CTS"))
    if (atoll(e) > 0) s.dotp_slice_cts = (uint64_t)atoll(e);
  s.hoist_keys = env_choice("SHELFI_HOIST_KEYS_PER_PASS", {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16}, 0);
  if (const char* e = getenv("SHELFI_WAVG_CHUNK_MIB"))
    if (atoll(e) > 0) s.wavg_chunk_mib = (uint64_t)atoll(e);
  if (const char* e = getenv("SHELFI_STAGE_SLOT_MIB"))
    if (atoll(e) > 0 && atoll(e) <= 256) s.stage_slot_mib = (uint64_t)atoll(e);
  s.h2d_direct = env_flag("SHELFI_H2D_DIRECT", '1', false);
  s.h2d_two = env_flag("SHELFI_H2D_TWO", '0', true);
  g_switches.store(new Switches(s), std::memory_order_release);
}
const Switches& switches() { return *g_switches.load(std::memory_order_acquire); }
static const bool g_switches_read = (reload_switches(), true);

}  // namespace shelfi

extern "C" {

void shelfi_reload_switches(void) { shelfi::reload_switches(); }

}  // extern "C"
