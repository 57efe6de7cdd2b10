// poly_plan.cpp — the host-only plan of EvalPoly: Paterson-Stockmeyer with four baby steps,
// p(x) = sum_g x^{4g} q_g(x), deg q_g <= 3.  The plan fixes which powers are computed and from what, every power's
// towers and exact scale, the level and scale the giant-step products are combined at, and the integer constants
// W_{g,j} = round(a_{4g+j} c_{g,j}) whose encoding scales c_{g,j} absorb each power's own scale -- so the terms of
// the combine all sit at S_c exactly, whatever the rescales of the powers did to theirs.  No device is touched.
//
// Every rule here is restated in Python ints and Fractions by tests/poly_ref.py and compared field for field.
#include <cmath>
#include <cstring>

#include "api_util.h"
#include "shelfi_internal.h"

using namespace shelfi;

namespace {

// a finite positive double as mant 2^exp, mant < 2^53 (0 for 0)
void split(double v, uint64_t* mant, int* exp) {
  int e;
  const double m = std::frexp(v, &e);  // v = m 2^e, m in [0.5, 1)
  *mant = (uint64_t)std::ldexp(m, 53);
  *exp = e - 53;
}

// little-endian words of an unsigned integer below 2^(64 kWords)
constexpr int kWords = 18;  // Q < 2^960 (16 towers below 2^60); 2 |W| is compared against it
struct Big {
  uint64_t w[kWords] = {0};
};

bool ge(const Big& a, const Big& b) {
  for (int i = kWords - 1; i >= 0; --i)
    if (a.w[i] != b.w[i]) return a.w[i] > b.w[i];
  return true;
}

// |W| = floor(|a| c + 1/2) for the exact product of the two doubles, as M 2^e with M < 2^106; false when 2 |W| >= Q
// (Q of `bits` bits, in `Q`).  res[t] = |W| mod q_t.
bool round_product(double a, double c, const uint64_t* q, uint32_t tc, const Big& Q, uint32_t bits, uint64_t* res) {
  uint64_t ma, mc;
  int ea, ec;
  split(a, &ma, &ea);
  split(c, &mc, &ec);
  const u128 M = (u128)ma * mc;
  const int e = ea + ec;
  Big W2;  // 2 |W|
  if (e >= 0) {
    if ((uint32_t)e + 1 >= bits) return false;  // M >= 1: 2 M 2^e >= 2^bits > Q (and W2 below stays inside kWords)
    const int sh = e + 1, wi = sh / 64, bi = sh % 64;
    const uint64_t lo = (uint64_t)M, hi = (uint64_t)(M >> 64);
    uint64_t part[3] = {lo << bi, bi ? (hi << bi) | (lo >> (64 - bi)) : hi, bi ? hi >> (64 - bi) : 0};
    for (int i = 0; i < 3; ++i) {
      if (wi + i < kWords) W2.w[wi + i] = part[i];
      else if (part[i]) return false;
    }
    if (ge(W2, Q)) return false;
    for (uint32_t t = 0; t < tc; ++t)
      res[t] = (uint64_t)(((u128)(uint64_t)(M % q[t]) * powmod(2, (uint64_t)e, q[t])) % q[t]);
    return true;
  }
  const int s = -e;  // |W| = floor((M + 2^(s-1)) / 2^s); M < 2^106
  const u128 R = s > 107 ? 0 : (M + ((u128)1 << (s - 1))) >> s;
  W2.w[0] = (uint64_t)(R << 1);
  W2.w[1] = (uint64_t)(R >> 63);
  if (ge(W2, Q)) return false;
  for (uint32_t t = 0; t < tc; ++t) res[t] = (uint64_t)(R % q[t]);
  return true;
}

bool good(double v) { return std::isfinite(v) && v > 0.0; }

}  // namespace

extern "C" int shelfi_poly_plan(uint32_t num_towers, const uint64_t* moduli, uint32_t scale_bits, const double* coeffs,
                                uint32_t degree, uint32_t towers, double scale, double combine_scale,
                                shelfi_poly_schedule* out) {
  if (!moduli || !coeffs || !out) return SHELFI_ERR_ARG;
  return guarded([&] {
    if (num_towers < 1 || num_towers > (uint32_t)kMaxTowers) throw Error{SHELFI_ERR_ARG, "poly_plan: 1..16 towers"};
    if (degree < 1 || degree > SHELFI_POLY_MAX_DEGREE) throw Error{SHELFI_ERR_ARG, "poly_plan: the degree must be 1..31"};
    for (uint32_t i = 0; i <= degree; ++i)
      if (!std::isfinite(coeffs[i])) throw Error{SHELFI_ERR_ARG, "poly_plan: non-finite coefficient"};
    if (towers < 1 || towers > num_towers) throw Error{SHELFI_ERR_ARG, "poly_plan: the input sits at 1..L towers"};
    if (scale_bits < 1 || scale_bits > 60) throw Error{SHELFI_ERR_ARG, "poly_plan: 1..60 scaling bits"};
    if (!good(scale) || !(combine_scale == 0.0 || good(combine_scale)))
      throw Error{SHELFI_ERR_ARG, "poly_plan: the scales must be finite and positive (combine scale 0: the default)"};
    for (uint32_t t = 0; t < num_towers; ++t)
      if (moduli[t] < 2 || moduli[t] >> 60) throw Error{SHELFI_ERR_ARG, "poly_plan: moduli in [2, 2^60)"};
    shelfi_poly_schedule pl;
    std::memset(&pl, 0, sizeof(pl));
    const uint32_t G = (degree + 4) / 4, nb = degree < 3 ? degree : 3, r = G > 1 ? 2 : 1;
    pl.degree = degree;
    pl.giants = G;
    pl.babies = nb;
    pl.rescales = r;
    // the schedule, in an order in which every factor comes before its product
    uint32_t tw[SHELFI_POLY_MAX_DEGREE + 1] = {0};  // towers of P_n, 0 = not computed
    double sc[SHELFI_POLY_MAX_DEGREE + 1] = {0};
    uint32_t np = 0;
    const auto put = [&](uint32_t n, uint32_t a, uint32_t b) {
      if (n == 1) {
        tw[1] = towers;
        sc[1] = scale;
      } else {
        const uint32_t t = tw[a] < tw[b] ? tw[a] : tw[b];  // the mult's level: the lower operand's
        if (t < 2) throw Error{SHELFI_ERR_ARG, "poly_plan: not enough levels for the powers"};
        tw[n] = t - 1;
        sc[n] = (sc[a] * sc[b]) / (double)moduli[t - 1];
        if (!good(sc[n])) throw Error{SHELFI_ERR_ARG, "poly_plan: a power's scale leaves the double range"};
      }
      pl.power_n[np] = n;
      pl.power_a[np] = a;
      pl.power_b[np] = b;
      pl.power_towers[np] = tw[n];
      pl.power_scale[np] = sc[n];
      ++np;
    };
    put(1, 0, 0);
    if (degree >= 2) put(2, 1, 1);
    if (degree >= 3) put(3, 2, 1);
    if (G > 1) put(4, 2, 2);
    for (uint32_t g = 2; g < G; ++g) {
      uint32_t h = 1;
      while (h * 2 < g) h *= 2;  // the largest power of two below g
      put(4 * g, 4 * h, 4 * (g - h));
    }
    pl.num_powers = np;
    uint32_t tc = towers;
    for (uint32_t i = 0; i < np; ++i) tc = pl.power_towers[i] < tc ? pl.power_towers[i] : tc;
    if (tc < r + 1) throw Error{SHELFI_ERR_ARG, "poly_plan: not enough levels for the combine's rescales"};
    const double Sc = combine_scale != 0.0 ? combine_scale : std::ldexp(1.0, (int)((G > 1 ? 3 : 2) * scale_bits));
    pl.combine_towers = tc;
    pl.combine_scale = Sc;
    Big Q;  // Q_{t_c}
    Q.w[0] = 1;
    for (uint32_t t = 0; t < tc; ++t) {
      u128 carry = 0;
      for (int i = 0; i < kWords; ++i) {
        const u128 v = (u128)Q.w[i] * moduli[t] + carry;
        Q.w[i] = (uint64_t)v;
        carry = v >> 64;
      }
    }
    uint32_t bits = 0;
    for (int i = kWords - 1; i >= 0 && !bits; --i)
      if (Q.w[i]) bits = 64 * (uint32_t)i + (64 - (uint32_t)__builtin_clzll(Q.w[i]));
    for (uint32_t g = 0; g < G; ++g)
      for (uint32_t j = 0; j < 4 && 4 * g + j <= degree; ++j) {
        double c = Sc;
        if (g) c = c / sc[4 * g];
        if (j) c = c / sc[j];
        if (!good(c)) throw Error{SHELFI_ERR_ARG, "poly_plan: a constant's scale leaves the double range"};
        pl.const_scale[g][j] = c;
        const double a = coeffs[4 * g + j];
        if (a == 0.0) continue;
        uint64_t res[kMaxTowers];
        if (!round_product(std::fabs(a), c, moduli, tc, Q, bits, res))
          throw Error{SHELFI_ERR_ARG, "poly_plan: a constant reaches Q / 2 at the combine level"};
        for (uint32_t t = 0; t < tc; ++t)
          pl.table[g][j][t] = (a < 0.0 && res[t]) ? moduli[t] - res[t] : res[t];
      }
    pl.result_towers = tc - r;
    double rs = Sc;
    for (uint32_t i = 0; i < r; ++i) rs = rs / (double)moduli[tc - 1 - i];
    pl.result_scale = rs;
    *out = pl;
  });
}
