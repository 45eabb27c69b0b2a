// wavefront_frame_check.cpp -- the Pauli frame of the wavefront pass
// (csrc/dtc_wf_frame.h, the code the prep kernel runs) on the CPU: a 12-bit
// tile goes through one launch's program twice,
//   directly: every kick's 2x2 matrix diag(1, sigma) S of its variant, the
//             partial diagonals from their two tables as given;
//   in frame form, as dtc_wavefront.hip does it: the form-B butterfly G(f^)
//             with the walk's coefficient for every site bit of a kicked
//             nibble, each diagonal's tables staged index-XORed by the frame's
//             X (and the last one's signed by its Z), i^ph on the whole tile,
//             the X flush at the store (index y written to y ^ x),
// and the two tiles must agree to 1e-12 (both scaled by the kicks' common
// 1 / sqrt(1 + coef^2), so the tile keeps norm 1).  The kernel stages only a
// slot's per-register table and has each thread fetch its own entry of the
// other table from the global one (wf_thr_fetch, wf_thr_neg, wf_reg_*): every
// such entry must equal the fully staged table's, bit for bit.
// Cases: RX and RY; tile 1 (all 12 bits are sites) and tile 2 (bits 0..2 are
// columns, never kicked); 1..4 steps, with and without the trailing diagonal,
// with and without the diagonal before step 0 (a pass that enters with that
// layer's factors applied; with one step and no trailing diagonal the launch
// has none at all, and the tile takes the frame's Z as a sign at the end);
// the junction bit (11 / 3) kicked in every step or in two consecutive ones
// only, and random masks; both values of the index bit outside the tile that
// a bond reaches.  Over the seeds every variant must occur on every site bit.
//
// Host only: c++ -std=c++17 -I <csrc> tools/wavefront_frame_check.cpp (it may
// also be built with -fsanitize=address,undefined and run as it is).
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "dtc_wf_frame.h"

namespace {

using cd = std::complex<double>;
constexpr int NB = dtc::kWfFrameBits, NS = dtc::kWfFrameSteps, NT = 1 << NB;
constexpr int kTabA = 128, kTabB = 64;  // tile bits 0..6 and 6..11

struct Case {
  bool rx;
  int act, n_steps, dmask, out;
  uint32_t mask[NS];
  int var[NS][NB];
  double coef[NS][NB];
  std::vector<cd> tab[NS + 1];  // kTabA + kTabB entries per diagonal
};

// diag(1, sigma) S of the variant on bit k (dtc_kernels.hip, SiteMat)
void kick_direct(std::vector<cd>& v, bool rx, int k, int var, double c) {
  const bool form_b = var & 2;
  const double sg = (var & 1) ? -1.0 : 1.0;
  const cd i1(0.0, 1.0);
  cd m00, m01, m10, m11;
  if (rx) {
    m00 = form_b ? c : 1.0; m01 = form_b ? i1 : i1 * c;
    m10 = m01; m11 = m00;
  } else {
    m00 = form_b ? c : 1.0; m01 = form_b ? 1.0 : c;
    m10 = -m01; m11 = m00;
  }
  m10 *= sg; m11 *= sg;
  for (int y = 0; y < NT; ++y) {
    if ((y >> k) & 1) continue;
    const cd u = v[y], w = v[y | (1 << k)];
    v[y] = m00 * u + m01 * w;
    v[y | (1 << k)] = m10 * u + m11 * w;
  }
}

// G(f) on bit k: RX f I + i X, RY f I + i Y (bfly_rx_f<2> / bfly_ry_f<2>)
void kick_g(std::vector<cd>& v, bool rx, int k, double f) {
  const cd i1(0.0, 1.0);
  for (int y = 0; y < NT; ++y) {
    if ((y >> k) & 1) continue;
    const cd u = v[y], w = v[y | (1 << k)];
    v[y] = rx ? f * u + i1 * w : f * u + w;
    v[y | (1 << k)] = rx ? f * w + i1 * u : f * w - u;
  }
}

// random nearest-neighbour phases: fields of all bits, the bonds among them,
// the bond of bit 11 to the outside bit (value `out`), split as the kernel's
// tables are (A: fields 0..5, bonds up to (5, 6); B: the rest)
std::vector<cd> make_tables(std::mt19937_64& rng, int out) {
  std::uniform_real_distribution<double> ang(-M_PI, M_PI);
  double h[NB], phi[NB];
  for (int k = 0; k < NB; ++k) h[k] = ang(rng), phi[k] = ang(rng);  // phi[11]: outside
  auto z = [](int y, int k) { return 1.0 - 2.0 * ((y >> k) & 1); };
  std::vector<cd> t(kTabA + kTabB);
  for (int a = 0; a < kTabA; ++a) {
    double e = 0.0;
    for (int k = 0; k < 6; ++k) e += h[k] * z(a, k) + phi[k] * z(a, k) * z(a, k + 1);
    t[a] = std::polar(1.0, -0.5 * e);
  }
  for (int b = 0; b < kTabB; ++b) {
    const int y = b << 6;
    double e = 0.0;
    for (int k = 6; k < NB; ++k) {
      e += h[k] * z(y, k);
      e += phi[k] * z(y, k) * (k + 1 < NB ? z(y, k + 1) : 1.0 - 2.0 * out);
    }
    t[kTabA + b] = std::polar(1.0, -0.5 * e);
  }
  return t;
}

// the kernel's order: even steps nibble 2, 1, 0, odd steps 0, 1, 2; fn(st, k)
// for every site bit of a nibble the step's mask touches
template <class F>
void for_step_bits(const Case& c, int st, F fn) {
  for (int i = 0; i < 3; ++i) {
    const int n = (st & 1) ? i : 2 - i;
    if (!(c.mask[st] & (0xFu << (4 * n)))) continue;
    for (int q = 0; q < 4; ++q)
      if ((c.act >> (4 * n + q)) & 1) fn(st, 4 * n + q);
  }
}

// fetch_fails: this case's direct-fetch / register-table entries that differ
// from the staged ones
double run_case(const Case& c, std::mt19937_64& rng, long& fetch_fails) {
  fetch_fails = 0;
  std::normal_distribution<double> nd;
  std::vector<cd> psi(NT);
  double nrm = 0.0;
  for (cd& a : psi) a = cd(nd(rng), nd(rng)), nrm += std::norm(a);
  for (cd& a : psi) a /= std::sqrt(nrm);

  double w = 1.0;  // the kicks' common scale
  std::vector<cd> ref = psi;
  for (int st = 0; st <= c.n_steps; ++st) {
    if ((c.dmask >> st) & 1)
      for (int y = 0; y < NT; ++y) ref[y] *= c.tab[st][y & (kTabA - 1)] * c.tab[st][kTabA + (y >> 6)];
    if (st == c.n_steps) break;
    for_step_bits(c, st, [&](int s, int k) {
      kick_direct(ref, c.rx, k, c.var[s][k], c.coef[s][k]);
      w /= std::sqrt(1.0 + c.coef[s][k] * c.coef[s][k]);
    });
  }

  dtc::WfFrame fr;
  dtc::wf_frame_walk(c.rx, c.n_steps, c.mask, c.dmask, c.act, c.var, c.coef, fr);
  int last = -1;  // the kernel's: the highest bit of dmask
  for (int st = 0; st <= c.n_steps; ++st)
    if ((c.dmask >> st) & 1) last = st;
  std::vector<cd> got = psi, stg(kTabA + kTabB);
  for (int st = 0; st <= c.n_steps; ++st) {
    if ((c.dmask >> st) & 1) {
      // the staging of dtc_wf_pass: entry i of a table goes to i ^ (its part of x)
      const int x = (int)(fr.xdiag >> (NB * st)) & (NT - 1);
      for (int t = 0; t < kTabA + kTabB; ++t) {
        const bool hi = t >= kTabA;
        const int ti = hi ? t - kTabA : t;
        const int j = ti ^ (hi ? x >> 6 : x & (kTabA - 1));
        const int zt = hi ? fr.zlast >> 6 : fr.zlast & 63;
        const bool neg = st == last && (__builtin_popcount(j & zt) & 1);
        stg[(hi ? kTabA : 0) + j] = neg ? -c.tab[st][t] : c.tab[st][t];
      }
      // dtc_wf_pass keeps only the slot's per-register table in LDS and each
      // thread fetches its own entry of the other from the global table
      // (wf_thr_fetch / wf_thr_neg): both must be the staged values, bit for
      // bit, in layout 2 (even slots) and in layout 0 (tile 1's odd slots; the
      // column tile's layout-1 pair: tools/wavefront_lay1_check.cpp)
      const int lay = (st & 1) ? 0 : 2;
      for (int t = 0; t < 256; ++t) {
        const int y = lay == 2 ? t : t << 4;  // ybase<lay>(t)
        cd e = c.tab[st][dtc::wf_thr_fetch(lay, y, x)];
        if (st == last && dtc::wf_thr_neg(lay, y, fr.zlast)) e = -e;
        const cd want = lay == 2 ? stg[y & (kTabA - 1)] : stg[kTabA + (y >> 6)];
        if (e != want) ++fetch_fails;
      }
      for (int i = 0; i < dtc::wf_reg_size(lay); ++i) {
        const int j = i ^ dtc::wf_reg_xmask(lay, x);
        const bool neg =
            st == last && (__builtin_popcount(j & dtc::wf_reg_zmask(lay, fr.zlast)) & 1);
        const cd e = c.tab[st][dtc::wf_reg_base(lay) + i];
        if ((neg ? -e : e) != stg[dtc::wf_reg_base(lay) + j]) ++fetch_fails;
      }
      for (int y = 0; y < NT; ++y) got[y] *= stg[y & (kTabA - 1)] * stg[kTabA + (y >> 6)];
    }
    if (st == c.n_steps) break;
    for_step_bits(c, st, [&](int s, int k) { kick_g(got, c.rx, k, fr.coef[s][k]); });
  }
  if (!c.dmask)  // no diagonal: the sign with the global factor, before the store
    for (int y = 0; y < NT; ++y)
      if (__builtin_popcount(y & fr.zlast) & 1) got[y] = -got[y];
  const cd ip[4] = {cd(1, 0), cd(0, 1), cd(-1, 0), cd(0, -1)};
  double err = 0.0;
  for (int y = 0; y < NT; ++y) {
    const double e = std::abs(w * (ip[fr.ph & 3] * got[y] - ref[y ^ fr.xend]));
    if (!(e <= err)) err = e;  // (a NaN stays)
  }
  return err;
}

}  // namespace

int main() {
  int cover[2][2][NB] = {};  // variants seen per (kind, tile, site bit)
  double worst = 0.0;
  long n_cases = 0;
  for (int rx = 0; rx < 2; ++rx)
    for (int tile = 0; tile < 2; ++tile) {
      const int act = tile ? 0xFF8 : 0xFFF, junction = tile ? 3 : 11;
      for (int n_steps = 1; n_steps <= NS; ++n_steps)
        for (int trailing = 0; trailing < 2; ++trailing)
          for (int mk = 0; mk < 5; ++mk)
            for (int seed = 0; seed < 8; ++seed) {
              const int first = (seed >> 1) & 1;  // the diagonal before step 0
              std::mt19937_64 rng(1000003ull * seed + 7919 * mk + 131 * n_steps + 17 * trailing +
                                  5 * tile + rx);
              std::uniform_real_distribution<double> cf(-1.0, 1.0);
              Case c;
              c.rx = rx;
              c.act = act;
              c.n_steps = n_steps;
              c.out = seed & 1;
              c.dmask = trailing << n_steps;
              for (int st = 0; st < NS; ++st) {
                uint32_t m = (uint32_t)act;
                // mk 1..3: the junction in steps (mk - 1, mk) only; mk 2 is the
                // steady pass's (steps 1 and 2); mk 4: random bits
                if (mk >= 1 && mk <= 3 && st != mk - 1 && st != mk) m &= ~(1u << junction);
                if (mk == 4) m &= (uint32_t)rng() | (1u << (4 + (int)(rng() % 8)));
                c.mask[st] = st < n_steps ? m : 0u;
                if (st < n_steps && (st || first)) c.dmask |= 1 << st;
                for (int k = 0; k < NB; ++k) {
                  const bool on = (c.mask[st] >> k) & 1;
                  // unkicked bits: the identity record
                  c.var[st][k] = on ? (int)(rng() & 3) : 0;
                  c.coef[st][k] = on ? cf(rng) : 0.0;
                  if (on) cover[rx][tile][k] |= 1 << c.var[st][k];
                }
              }
              for (int st = 0; st <= NS; ++st) c.tab[st] = make_tables(rng, c.out);
              long fetch_fails = 0;
              const double err = run_case(c, rng, fetch_fails);
              ++n_cases;
              if (err > worst) worst = err;
              if (fetch_fails) {
                std::printf("FAIL rx %d tile %d steps %d dmask %d masks %d seed %d: %ld fetched "
                            "table entries differ from the staged ones\n", rx, tile, n_steps,
                            c.dmask, mk, seed, fetch_fails);
                return 1;
              }
              if (!(err < 1e-12)) {
                std::printf("FAIL rx %d tile %d steps %d dmask %d masks %d seed %d: %.3e\n", rx,
                            tile, n_steps, c.dmask, mk, seed, err);
                return 1;
              }
            }
      for (int k = 0; k < NB; ++k)
        if (((act >> k) & 1) && cover[rx][tile][k] != 15) {
          std::printf("FAIL coverage: rx %d tile %d bit %d saw variants 0x%x\n", rx, tile, k,
                      cover[rx][tile][k]);
          return 1;
        }
    }
  std::printf("wavefront frames: ok (%ld cases, worst %.3e)\n", n_cases, worst);
  return 0;
}
