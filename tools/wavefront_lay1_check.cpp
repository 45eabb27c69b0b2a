// wavefront_lay1_check.cpp -- the column tile's partial diagonal in layout 1
// (csrc/dtc_wf_frame.h: the register table over tile bits 3..8 and the thread
// table over bits 3, 8..11 that dtc_wavefront.hip looks up in the tile's odd
// steps and wf_table_set fills) on the CPU, for random fields and bonds of the
// tile's sites (tile bits 3..11; bits 0..2 are columns) and the bond from bit 3
// to the index bit outside the tile:
//  1. the product register table x thread table equals the product of the
//     0..6 and 6..11 tables of the three-layout form for every tile index, both
//     values of the outside bit, plain and conjugated (1e-14: the same angles
//     summed in another grouping);
//  2. staged under a frame -- entry i at i ^ (X gathered onto the table's index
//     bits), signed by the parity of the staged index under the gathered Z mask
//     -- a lookup at y gives (-1)^|y & z| D(y ^ x), exactly for the pair's own
//     product and to 1e-14 against the three-layout form staged its way; and
//     the kernel's split of every slot -- register table staged, the thread's
//     entry of the other table fetched from the global slot with the XOR and
//     the sign applied by the thread -- reproduces those staged tables exactly,
//     in layouts 2, 1 and 0;
//  3. the two-layout program (2 -> 1 in even steps, 1 -> 2 in odd ones, bit 3
//     kicked as an ordinary butterfly: across lanes it is the same fma per
//     amplitude) against the three-layout snake on a 12-bit tile: bit for bit
//     when only even steps carry a diagonal (the same arithmetic), to 1e-14 of
//     the tile's largest amplitude otherwise.
//
// Host only: c++ -std=c++17 -I <csrc> tools/wavefront_lay1_check.cpp (it may
// also be built with -fsanitize=address,undefined and run as it is).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "dtc_wf_frame.h"

namespace {

struct c2 {
  double x, y;
};
c2 cmul(c2 a, c2 b) { return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }

constexpr int NB = dtc::kWfFrameBits, NT = 1 << NB, NS = dtc::kWfFrameSteps;
constexpr int kTabA = 128, kTabB = 64;

struct Angles {
  double h[NB];     // field of tile bit k (3..11)
  double p[NB];     // bond (k, k + 1), k = 3..10
  double pout;      // bond from bit 3 to the outside bit
};

double zsign(int v, int pos) { return (pos >= 0 && ((v >> pos) & 1)) ? -1.0 : 1.0; }

// the three-layout form (wf_table_set): bits k <= 5 in the 0..6 table
void build_ab(const Angles& a, double zout, double sgn, std::vector<c2>& ta, std::vector<c2>& tb) {
  ta.assign(kTabA, {1.0, 0.0});
  tb.assign(kTabB, {1.0, 0.0});
  for (int half = 0; half < 2; ++half) {
    const int bit0 = half ? 6 : 0, n = half ? kTabB : kTabA;
    for (int v = 0; v < n; ++v) {
      double ang = 0.0;
      for (int k = 3; k < NB; ++k)
        if ((k <= 5) == (half == 0)) ang += a.h[k] * zsign(v, k - bit0);
      for (int k = 3; k + 1 < NB; ++k)
        if ((k <= 5) == (half == 0)) ang += a.p[k] * zsign(v, k - bit0) * zsign(v, k + 1 - bit0);
      if (half == 0) ang += a.pout * zsign(v, 3) * zout;
      (half ? tb : ta)[v] = {std::cos(sgn * ang), std::sin(sgn * ang)};
    }
  }
}

// the layout-1 pair, by the header's rules (as wf_table_set fills it)
void build_l1(const Angles& a, double zout, double sgn, std::vector<c2>& tr, std::vector<c2>& tt) {
  tr.assign(dtc::kWfL1Reg, {1.0, 0.0});
  tt.assign(dtc::kWfL1Thr, {1.0, 0.0});
  for (int half = 0; half < 2; ++half) {
    const int n = half ? dtc::kWfL1Thr : dtc::kWfL1Reg;
    auto pos = [&](int k) { return half ? dtc::wf_l1_thr_pos(k) : dtc::wf_l1_reg_pos(k); };
    for (int v = 0; v < n; ++v) {
      double ang = 0.0;
      for (int k = 3; k < NB; ++k)
        if (dtc::wf_l1_in_reg(k, -1) == (half == 0)) ang += a.h[k] * zsign(v, pos(k));
      for (int k = 3; k + 1 < NB; ++k)
        if (dtc::wf_l1_in_reg(k, k + 1) == (half == 0))
          ang += a.p[k] * zsign(v, pos(k)) * zsign(v, pos(k + 1));
      if (dtc::wf_l1_in_reg(3, -1) == (half == 0)) ang += a.pout * zsign(v, pos(3)) * zout;
      (half ? tt : tr)[v] = {std::cos(sgn * ang), std::sin(sgn * ang)};
    }
  }
}

int parity(int x) { return __builtin_popcount((unsigned)x) & 1; }

// staged copy: entry i at i ^ xm, negated where the staged index has odd
// parity under zm
std::vector<c2> stage(const std::vector<c2>& t, int xm, int zm) {
  std::vector<c2> s(t.size());
  for (int i = 0; i < (int)t.size(); ++i) {
    const int j = i ^ xm;
    s[j] = parity(j & zm) ? c2{-t[i].x, -t[i].y} : t[i];
  }
  return s;
}

// bfly_rx_f<2> / bfly_ry_f<2> on tile bit k
void kick(std::vector<c2>& v, bool rx, int k, double f) {
  for (int y = 0; y < NT; ++y) {
    if ((y >> k) & 1) continue;
    const c2 u = v[y], w = v[y | (1 << k)];
    if (rx) {
      v[y] = {std::fma(f, u.x, -w.y), std::fma(f, u.y, w.x)};
      v[y | (1 << k)] = {std::fma(f, w.x, -u.y), std::fma(f, w.y, u.x)};
    } else {
      v[y] = {std::fma(f, u.x, w.x), std::fma(f, u.y, w.y)};
      v[y | (1 << k)] = {std::fma(f, w.x, -u.x), std::fma(f, w.y, -u.y)};
    }
  }
}

// v[y] *= (fac * TC[..]) * TR[..]: wf_diag's shape, thread-constant table first
enum Form { kLay2, kLay0, kLay1 };
void diag(std::vector<c2>& v, Form form, const std::vector<c2>& t0, const std::vector<c2>& t1, c2 fac) {
  for (int y = 0; y < NT; ++y) {
    c2 c, e;
    if (form == kLay2) {
      c = cmul(fac, t0[y & (kTabA - 1)]);
      e = t1[y >> 6];
    } else if (form == kLay0) {
      c = cmul(fac, t1[y >> 6]);
      e = t0[y & (kTabA - 1)];
    } else {
      c = cmul(fac, t1[dtc::wf_l1_thr_index(y)]);
      e = t0[dtc::wf_l1_reg_index(y)];
    }
    v[y] = cmul(v[y], cmul(c, e));
  }
}

int fails = 0;
void want(bool ok, const char* what, int seed, double got) {
  if (ok) return;
  if (fails++ < 20) std::printf("FAIL seed %d: %s (%.3e)\n", seed, what, got);
}

double dist(c2 a, c2 b) { return std::hypot(a.x - b.x, a.y - b.y); }

}  // namespace

int main() {
  int n_prog = 0, n_exact = 0;
  double worst_tab = 0.0, worst_stage = 0.0, worst_prog = 0.0;
  for (int seed = 0; seed < 48; ++seed) {
    std::mt19937_64 rng(1000 + seed);
    std::uniform_real_distribution<double> ang(-M_PI, M_PI), bond(-1.5 * M_PI, -0.5 * M_PI),
        cf(-2.0, 2.0);
    Angles a;
    std::memset(&a, 0, sizeof a);
    for (int k = 3; k < NB; ++k) a.h[k] = ang(rng);
    for (int k = 3; k + 1 < NB; ++k) a.p[k] = bond(rng);
    a.pout = bond(rng);
    const double zout = (seed & 1) ? -1.0 : 1.0, sgn = (seed & 2) ? 0.5 : -0.5;
    std::vector<c2> ta, tb, tr, tt;
    build_ab(a, zout, sgn, ta, tb);
    build_l1(a, zout, sgn, tr, tt);

    // 1. the same diagonal
    for (int y = 0; y < NT; ++y) {
      const c2 d0 = cmul(ta[y & (kTabA - 1)], tb[y >> 6]);
      const c2 d1 = cmul(tr[dtc::wf_l1_reg_index(y)], tt[dtc::wf_l1_thr_index(y)]);
      const double e = dist(d0, d1);
      worst_tab = std::fmax(worst_tab, e);
      want(e < 1e-14, "layout-1 product != 0..6 x 6..11 product", seed, e);
    }

    // 2. staged under a frame (masks on the tile's site bits 3..11)
    const int fx = (int)(rng() & (NT - 1)) & ~7, fz = (int)(rng() & (NT - 1)) & ~7;
    {
      const std::vector<c2> sr = stage(tr, dtc::wf_l1_reg_index(fx), dtc::wf_l1_reg_zmask(fz));
      const std::vector<c2> st = stage(tt, dtc::wf_l1_thr_index(fx), dtc::wf_l1_thr_zmask(fz));
      const std::vector<c2> sa = stage(ta, fx & (kTabA - 1), fz & 63);
      const std::vector<c2> sb = stage(tb, fx >> 6, fz >> 6);
      for (int y = 0; y < NT; ++y) {
        const c2 got = cmul(sr[dtc::wf_l1_reg_index(y)], st[dtc::wf_l1_thr_index(y)]);
        const int x = y ^ fx;
        c2 ref = cmul(tr[dtc::wf_l1_reg_index(x)], tt[dtc::wf_l1_thr_index(x)]);
        if (parity(y & fz)) ref = {-ref.x, -ref.y};
        want(got.x == ref.x && got.y == ref.y, "staged lookup != signed, permuted diagonal", seed,
             dist(got, ref));
        const c2 old = cmul(sa[y & (kTabA - 1)], sb[y >> 6]);
        const double e = dist(got, old);
        worst_stage = std::fmax(worst_stage, e);
        want(e < 1e-14, "staged layout-1 pair != staged 0..6 x 6..11 pair", seed, e);
      }
      // the kernel's split of a slot: the per-register table staged in LDS
      // (wf_reg_*), the thread's own entry of the other fetched from the
      // slot's global table (wf_thr_fetch / wf_thr_neg) -- both are the staged
      // values above, bit for bit, in all three layouts
      auto same = [](c2 a, c2 b) { return a.x == b.x && a.y == b.y; };
      for (int lay = 0; lay < 3; ++lay) {
        std::vector<c2> slot = lay == 1 ? tr : ta;  // the slot as wf_table_set fills it
        const std::vector<c2>& second = lay == 1 ? tt : tb;
        slot.insert(slot.end(), second.begin(), second.end());
        const std::vector<c2>& sreg = lay == 1 ? sr : (lay == 2 ? sb : sa);
        for (int t = 0; t < 256; ++t) {
          const int y = lay == 2 ? t : (lay == 1 ? ((t & 15) | ((t >> 4) << 8)) : t << 4);
          c2 e = slot[dtc::wf_thr_fetch(lay, y, fx)];
          if (dtc::wf_thr_neg(lay, y, fz)) e = {-e.x, -e.y};
          const c2 ref = lay == 1   ? st[dtc::wf_l1_thr_index(y)]
                         : lay == 2 ? sa[y & (kTabA - 1)]
                                    : sb[y >> 6];
          want(same(e, ref), "fetched thread entry != staged thread table", seed, dist(e, ref));
        }
        want((int)sreg.size() == dtc::wf_reg_size(lay), "register table size", seed, lay);
        for (int i = 0; i < dtc::wf_reg_size(lay); ++i) {
          const int j = i ^ dtc::wf_reg_xmask(lay, fx);
          c2 e = slot[dtc::wf_reg_base(lay) + i];
          if (parity(j & dtc::wf_reg_zmask(lay, fz))) e = {-e.x, -e.y};
          want(same(e, sreg[j]), "staged register table != staged table", seed, dist(e, sreg[j]));
        }
      }
    }

    // 3. the programs: n steps, diagonals per dmask (bit n: the trailing one)
    for (int rx = 0; rx < 2; ++rx) {
      for (int n = 1; n <= NS; ++n) {
        const int dmask = (seed % 3 == 0) ? (0x15 & ((2 << n) - 1))  // even slots only
                                          : ((int)(rng() & 31) & ((2 << n) - 1));
        uint32_t mask[NS];
        double f[NS][NB];
        std::vector<c2> tabs[NS + 1][4];
        for (int s = 0; s <= NS; ++s) {
          Angles b = a;
          for (int k = 3; k < NB; ++k) b.h[k] = ang(rng);
          build_ab(b, zout, sgn, tabs[s][0], tabs[s][1]);
          build_l1(b, zout, sgn, tabs[s][2], tabs[s][3]);
        }
        for (int s = 0; s < NS; ++s) {
          mask[s] = (uint32_t)(rng() & (NT - 1)) & ~7u;
          if (seed & 4) mask[s] |= 8u;  // the junction bit in every step
          for (int k = 0; k < NB; ++k) f[s][k] = ((mask[s] >> k) & 1) ? cf(rng) : 0.0;
        }
        std::vector<c2> v0(NT), v1;
        for (c2& z : v0) z = {cf(rng), cf(rng)};
        v1 = v0;
        const c2 g = {std::cos(0.3 + seed), std::sin(0.3 + seed)};
        for (int prog = 0; prog < 2; ++prog) {
          std::vector<c2>& v = prog ? v1 : v0;
          c2 fac = g;
          auto dg = [&](int s) {
            if (!((dmask >> s) & 1)) return;
            if (!(s & 1)) diag(v, kLay2, tabs[s][0], tabs[s][1], fac);
            else if (prog) diag(v, kLay1, tabs[s][2], tabs[s][3], fac);
            else diag(v, kLay0, tabs[s][0], tabs[s][1], fac);
            fac = {1.0, 0.0};
          };
          // a kicked nibble runs all its site bits (an unkicked one: f = 0)
          auto nib = [&](int s, int nb) {
            if (!(mask[s] & (0xFu << (4 * nb)))) return;
            for (int q = (nb ? 0 : 3); q < 4; ++q) kick(v, rx, 4 * nb + q, f[s][4 * nb + q]);
          };
          for (int s = 0; s < n; ++s) {
            dg(s);
            if (!(s & 1)) { nib(s, 2); nib(s, 1); nib(s, 0); }
            else { nib(s, 0); nib(s, 1); nib(s, 2); }
          }
          dg(n);
        }
        double top = 0.0, e = 0.0;
        bool same = true;
        for (int y = 0; y < NT; ++y) {
          top = std::fmax(top, std::hypot(v0[y].x, v0[y].y));
          e = std::fmax(e, dist(v0[y], v1[y]));
          same = same && v0[y].x == v1[y].x && v0[y].y == v1[y].y;
        }
        ++n_prog;
        if (!(dmask & 0xA)) {
          ++n_exact;
          want(same, "programs differ without an odd-step diagonal", seed, e / top);
        }
        worst_prog = std::fmax(worst_prog, e / top);
        want(e <= 1e-14 * top, "two-layout program != three-layout snake", seed, e / top);
      }
    }
  }
  std::printf("tables %.2e  staged %.2e  programs %.2e (%d, %d bit for bit)\n", worst_tab,
              worst_stage, worst_prog, n_prog, n_exact);
  if (fails || n_exact < 16 || n_exact == n_prog) {
    std::printf("wavefront lay1: FAILED (%d)\n", fails);
    return 1;
  }
  std::printf("wavefront lay1: ok\n");
  return 0;
}
