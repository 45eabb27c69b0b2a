// wavefront_t1_swap_check.cpp -- tile 1's swap form of the wavefront pass
// (csrc/dtc_wavefront.hip, DTC_WF_T1_SWAP; the layouts L2, L2s, Q, Qs and the
// slot map of csrc/dtc_wf_frame.h) on the CPU, thread by thread and register by
// register as the kernel holds the tile:
//  (a) index bookkeeping: the four thread / register -> tile index maps and the
//      slot map are permutations; the row swaps (the permlane semantics of
//      swap_rows) turn L2 into L2s and Q into Qs; the three LDS re-layouts
//      L2s -> Qs, Qs -> L2s, Q -> L2 land every index where the target layout
//      wants it; a step pair and an odd-length pass compose to the identity;
//      every site is a register bit where the program kicks it; the table
//      indices used in Q are layout 0's for the same tile index; a thread
//      writes only slots it read itself in the re-layout before, except in
//      Q -> L2, which the kernel runs behind a barrier.
//  (b) bank conflicts: every store (16-lane groups, banks (a / 4) mod 32) and
//      every load (32-lane groups, banks (a / 4) mod 64) of the three maps
//      touches no bank twice, over all waves and registers.
//      Likewise layout 0's register table in rows of 17 (wf_pad0) under
//      ds_read_b128's lane groups, for the snake's layout 0 and for Q; rows of
//      16 must show the conflict, so the check is known to see one.
//  (c) the program: a random tile through the swap form -- swaps, re-layouts
//      through a 4096-slot buffer, butterflies on register bits, diagonals
//      from the staged register table and the fetched thread entry -- equals,
//      bit for bit, the frame-form model of tools/wavefront_frame_check.cpp on
//      the tile index (kicks of a layer in the swap form's order in both).
//      RX and RY, 1..4 steps, with and without the trailing and the leading
//      diagonal, the steady pass's masks (junction bit 11 in steps 1, 2 only),
//      the ramps' and random ones.
//
// Host only: c++ -std=c++17 -I <csrc> tools/wavefront_t1_swap_check.cpp (it
// may also be built with -fsanitize=address,undefined and run as it is).
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "dtc_wf_frame.h"

namespace {

using cd = std::complex<double>;
constexpr int NB = dtc::kWfFrameBits, NS = dtc::kWfFrameSteps, NT = 1 << NB;
constexpr int kThreads = 256, kRegs = 16, kSlots = 4096;
constexpr int kTabA = 128, kTabB = 64;
using dtc::kWfLayL2;
using dtc::kWfLayL2s;
using dtc::kWfLayQ;
using dtc::kWfLayQs;

int yof(int lay, int t, int r) { return dtc::wf_t1_ybase(lay, t) ^ dtc::wf_t1_roff(lay, r); }

#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      std::printf("FAIL " __VA_ARGS__); \
      std::printf("\n");            \
      return false;                 \
    }                               \
  } while (0)

// The tile as the workgroup holds it: v[t][r].
template <class T>
struct Regs {
  std::vector<T> a = std::vector<T>(kThreads * kRegs);
  T& operator()(int t, int r) { return a[t * kRegs + r]; }
  const T& operator()(int t, int r) const { return a[t * kRegs + r]; }
};

// swap_reg_lane<Q, M>: per register pair (bit Q clear / set) the permlane swap
// of swap_rows -- the first keeps its lanes without lane bit M and takes the
// second's from the partner lane, the second likewise with the bit set
template <class T>
void swap_reg_lane(Regs<T>& v, int q, int m) {
  Regs<T> o = v;
  for (int t = 0; t < kThreads; ++t)
    for (int r = 0; r < kRegs; ++r) {
      if (r & (1 << q)) continue;
      const int r1 = r | (1 << q);
      const bool up = t & m;
      v(t, r) = up ? o(t ^ m, r1) : o(t, r);
      v(t, r1) = up ? o(t, r1) : o(t ^ m, r);
    }
}
template <class T>
void t1_swap(Regs<T>& v) {
  swap_reg_lane(v, 0, 16);
  swap_reg_lane(v, 1, 32);
}

// exchange_t1<from, to>; owner (per slot: the thread that read it last, -1
// before any read) checks the write rule when `rule` is set
template <class T>
bool exchange(Regs<T>& v, int from, int to, std::vector<int>& owner, bool rule) {
  std::vector<T> buf(kSlots);
  std::vector<char> hit(kSlots, 0);
  for (int t = 0; t < kThreads; ++t)
    for (int r = 0; r < kRegs; ++r) {
      const int s = dtc::wf_t1_slot(dtc::wf_t1_ybase(from, t)) ^
                    dtc::wf_t1_slot(dtc::wf_t1_roff(from, r));
      CHECK(s >= 0 && s < kSlots && !hit[s], "re-layout %d -> %d: slot %d", from, to, s);
      CHECK(!rule || owner[s] < 0 || owner[s] == t,
            "re-layout %d -> %d: thread %d writes slot %d that thread %d read", from, to, t, s,
            owner[s]);
      hit[s] = 1;
      buf[s] = v(t, r);
    }
  for (int t = 0; t < kThreads; ++t)
    for (int r = 0; r < kRegs; ++r) {
      const int s = dtc::wf_t1_slot(dtc::wf_t1_ybase(to, t)) ^
                    dtc::wf_t1_slot(dtc::wf_t1_roff(to, r));
      CHECK(s >= 0 && s < kSlots, "re-layout %d -> %d: slot %d", from, to, s);
      v(t, r) = buf[s];
      owner[s] = t;
    }
  return true;
}

bool holds_layout(const Regs<int>& v, int lay, const char* what) {
  for (int t = 0; t < kThreads; ++t)
    for (int r = 0; r < kRegs; ++r)
      CHECK(v(t, r) == yof(lay, t, r), "%s: thread %d register %d holds index %d, layout %d wants %d",
            what, t, r, v(t, r), lay, yof(lay, t, r));
  return true;
}

bool check_indices() {
  // the maps are permutations, linear in (t, r)
  for (int lay = 0; lay < 4; ++lay) {
    std::vector<char> seen(NT, 0);
    for (int t = 0; t < kThreads; ++t)
      for (int r = 0; r < kRegs; ++r) {
        const int y = yof(lay, t, r);
        CHECK((dtc::wf_t1_ybase(lay, t) & dtc::wf_t1_roff(lay, r)) == 0, "layout %d: base and offset overlap", lay);
        CHECK(y >= 0 && y < NT && !seen[y], "layout %d: index %d twice", lay, y);
        seen[y] = 1;
      }
  }
  {
    std::vector<char> seen(kSlots, 0);
    for (int y = 0; y < NT; ++y) {
      const int s = dtc::wf_t1_slot(y);
      CHECK(s >= 0 && s < kSlots && !seen[s], "slot map: slot %d twice", s);
      seen[s] = 1;
      for (int k = 0; k < NB; ++k)
        CHECK((dtc::wf_t1_slot(y ^ (1 << k)) ^ s) == dtc::wf_t1_slot(1 << k), "slot map: not linear");
    }
  }
  // sites in registers where the program kicks them
  const int site[4][4] = {{8, 9, 10, 11}, {4, 5, -1, -1}, {0, 1, 2, 3}, {6, 7, -1, -1}};
  for (int lay = 0; lay < 4; ++lay)
    for (int q = 0; q < 4; ++q)
      if (site[lay][q] >= 0)
        CHECK(dtc::wf_t1_roff(lay, 1 << q) == 1 << site[lay][q], "layout %d: register bit %d is not site %d",
              lay, q, site[lay][q]);
  // L2 is the load / store layout of the kernel: y = t | r << 8
  for (int t = 0; t < kThreads; ++t)
    for (int r = 0; r < kRegs; ++r) CHECK(yof(kWfLayL2, t, r) == (t | (r << 8)), "L2 is not layout 2");

  // a step pair, then a third step and the way back of an odd-length pass
  Regs<int> v;
  std::vector<int> owner(kSlots, -1);
  for (int t = 0; t < kThreads; ++t)
    for (int r = 0; r < kRegs; ++r) v(t, r) = yof(kWfLayL2, t, r);
  for (int rep = 0; rep < 2; ++rep) {
    t1_swap(v);
    if (!holds_layout(v, kWfLayL2s, "swap L2 -> L2s")) return false;
    if (!exchange(v, kWfLayL2s, kWfLayQs, owner, true)) return false;
    if (!holds_layout(v, kWfLayQs, "L2s -> Qs")) return false;
    t1_swap(v);
    if (!holds_layout(v, kWfLayQ, "swap Qs -> Q")) return false;
    if (rep == 1) break;
    t1_swap(v);
    if (!holds_layout(v, kWfLayQs, "swap Q -> Qs")) return false;
    if (!exchange(v, kWfLayQs, kWfLayL2s, owner, true)) return false;
    if (!holds_layout(v, kWfLayL2s, "Qs -> L2s")) return false;
    t1_swap(v);
    if (!holds_layout(v, kWfLayL2, "swap L2s -> L2 (a step pair is the identity)")) return false;
  }
  {
    // Q -> L2 writes from Q what came back in Qs: other threads' slots (the
    // kernel's barrier in front of it), all of them in the thread's own wave
    for (int t = 0; t < kThreads; ++t)
      for (int r = 0; r < kRegs; ++r) {
        const int s = dtc::wf_t1_slot(yof(kWfLayQ, t, r));
        CHECK((owner[s] >> 6) == (t >> 6), "Q -> L2: thread %d writes a slot of another wave", t);
      }
    if (!exchange(v, kWfLayQ, kWfLayL2, owner, false)) return false;
    if (!holds_layout(v, kWfLayL2, "Q -> L2 (an odd-length pass is the identity)")) return false;
    // the next pass's first re-layout writes before anybody has read
  }

  // the tables' indices in Q are layout 0's for the same tile index
  for (int t = 0; t < kThreads; ++t) {
    const int yb = dtc::wf_t1_ybase(kWfLayQ, t);
    for (int r = 0; r < kRegs; ++r) {
      const int y = yof(kWfLayQ, t, r);
      const int t0 = y >> 4, r0 = y & 15;  // layout 0: ybase<0>(t0) = t0 << 4
      CHECK(r0 == r, "Q: register %d holds tile bits 0..3 = %d", r, r0);
      CHECK((yb & 0x70) + r == ((t0 & 7) << 4) + r0 && (yb & 0x70) + r == (y & (kTabA - 1)),
            "Q: register-table index of tile index %d", y);
      CHECK(dtc::wf_thr_staged(0, yb) == dtc::wf_thr_staged(0, t0 << 4) &&
                dtc::wf_thr_staged(0, yb) == (y >> 6),
            "Q: thread-table index of tile index %d", y);
      for (int fx : {0, 0xFFF, 0x5A5, 0xA5A, 0x0C0, 0x800}) {
        CHECK(dtc::wf_thr_fetch(0, yb, fx) == dtc::wf_thr_fetch(0, t0 << 4, fx), "Q: wf_thr_fetch");
        CHECK(dtc::wf_thr_neg(0, yb, fx) == dtc::wf_thr_neg(0, t0 << 4, fx), "Q: wf_thr_neg");
      }
    }
  }
  return true;
}

// One wave instruction of a re-layout: the 64 lanes' slots.  8-B accesses at
// byte address 8 slot: dwords 2 slot, 2 slot + 1.
bool conflict_free(const int (&slot)[64], int group, int banks, const char* what, int lay, int w, int r) {
  for (int g = 0; g < 64; g += group) {
    std::vector<int> addr(banks, -1);
    for (int i = g; i < g + group; ++i)
      for (int d = 0; d < 2; ++d) {
        const int dw = 2 * slot[i] + d, bk = dw % banks;
        CHECK(addr[bk] < 0 || addr[bk] == dw, "%s of layout %d, wave %d, register %d, lanes %d..%d: bank %d twice",
              what, lay, w, r, g, g + group - 1, bk);
        addr[bk] = dw;
      }
  }
  return true;
}

bool check_banks(long& n_instr) {
  const int maps[3][2] = {{kWfLayL2s, kWfLayQs}, {kWfLayQs, kWfLayL2s}, {kWfLayQ, kWfLayL2}};
  for (const auto& m : maps)
    for (int side = 0; side < 2; ++side)
      for (int w = 0; w < kThreads / 64; ++w)
        for (int r = 0; r < kRegs; ++r) {
          int slot[64];
          for (int l = 0; l < 64; ++l)
            slot[l] = dtc::wf_t1_slot(dtc::wf_t1_ybase(m[side], w * 64 + l)) ^
                      dtc::wf_t1_slot(dtc::wf_t1_roff(m[side], r));
          // stores: 4 x 16 contiguous lanes, 32 banks; loads: 2 x 32 lanes, 64 banks
          if (!(side == 0 ? conflict_free(slot, 16, 32, "store", m[side], w, r)
                          : conflict_free(slot, 32, 64, "load", m[side], w, r)))
            return false;
          ++n_instr;
        }
  return true;
}

// Layout 0's diagonal reads its register table with ds_read_b128 (16-B entries,
// 4 x 16 lanes in the guide's groups, banks (a / 4) mod 64): the most distinct
// addresses that meet on one bank in a lane group, over waves and registers,
// for the thread maps of the snake's layout 0 (tile bits 4..6 = t & 7) and of Q
int table_read_ways(bool padded, bool q_map) {
  const int groups[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                             {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                             {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                             {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
  int worst = 0;
  for (int w = 0; w < kThreads / 64; ++w)
    for (int r = 0; r < kRegs; ++r)
      for (const auto& g : groups) {
        std::vector<std::vector<int>> on(64);  // distinct entries per bank
        for (int l : g) {
          const int t = w * 64 + l;
          const int row = q_map ? (dtc::wf_t1_ybase(kWfLayQ, t) & 0x70) : ((t & 7) << 4);
          const int e = (padded ? dtc::wf_pad0(row) : row) + r;
          for (int d = 0; d < 4; ++d) {
            std::vector<int>& b = on[(4 * e + d) % 64];
            bool seen = false;
            for (int x : b) seen = seen || x == e;
            if (!seen) b.push_back(e);
          }
        }
        for (const auto& b : on) worst = std::max(worst, (int)b.size());
      }
  return worst;
}

bool check_table_reads() {
  for (int q = 0; q < 2; ++q) {
    CHECK(table_read_ways(true, q) == 1, "layout 0's table in rows of 17 (%s): %d-way bank conflict",
          q ? "Q" : "snake", table_read_ways(true, q));
    CHECK(table_read_ways(false, q) > 1, "rows of 16 should conflict (%s): the check sees nothing", q ? "Q" : "snake");
  }
  CHECK(dtc::wf_pad0(dtc::kWfFetchTabA - 1) < dtc::kWfTabA0, "kWfTabA0 holds the padded table");
  for (int j = 1; j < dtc::kWfFetchTabA; ++j)
    CHECK(dtc::wf_pad0(j) > dtc::wf_pad0(j - 1), "wf_pad0 is not increasing at %d", j);
  return true;
}

// ---- (c) the program ----------------------------------------------------------
struct Case {
  bool rx;
  int n_steps, dmask, out;
  uint32_t mask[NS];
  int var[NS][NB];
  double coef[NS][NB];
  std::vector<cd> tab[NS + 1];  // kTabA + kTabB entries per diagonal
};

// G(f) of two amplitudes (tools/wavefront_frame_check.cpp, kick_g)
void bfly(bool rx, double f, cd& u, cd& w) {
  const cd i1(0.0, 1.0), a = u, b = w;
  u = rx ? f * a + i1 * b : f * a + b;
  w = rx ? f * b + i1 * a : f * b - a;
}

std::vector<cd> make_tables(std::mt19937_64& rng, int out) {
  std::uniform_real_distribution<double> ang(-M_PI, M_PI);
  double h[NB], phi[NB];
  for (int k = 0; k < NB; ++k) h[k] = ang(rng), phi[k] = ang(rng);
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

// the swap form's order of a step's sites: even steps 8..11, 4, 5, 6, 7, 0..3,
// odd steps 0..3, 6, 7, 4, 5, 8..11; a nibble runs whole or not at all
std::vector<int> step_sites(const Case& c, int st) {
  const int even[NB] = {8, 9, 10, 11, 4, 5, 6, 7, 0, 1, 2, 3};
  const int odd[NB] = {0, 1, 2, 3, 6, 7, 4, 5, 8, 9, 10, 11};
  std::vector<int> o;
  for (int i = 0; i < NB; ++i) {
    const int k = (st & 1) ? odd[i] : even[i];
    if (c.mask[st] & (0xFu << (4 * (k >> 2)))) o.push_back(k);
  }
  return o;
}

bool run_case(const Case& c, std::mt19937_64& rng) {
  std::normal_distribution<double> nd;
  std::vector<cd> psi(NT);
  for (cd& a : psi) a = cd(nd(rng), nd(rng)) / 64.0;

  dtc::WfFrame fr;
  dtc::wf_frame_walk(c.rx, c.n_steps, c.mask, c.dmask, 0xFFF, c.var, c.coef, fr);
  int last = -1;
  for (int st = 0; st <= c.n_steps; ++st)
    if ((c.dmask >> st) & 1) last = st;
  const int n = c.n_steps;

  // the model on the tile index: fully staged tables
  std::vector<cd> ref = psi;
  for (int st = 0; st <= n; ++st) {
    if ((c.dmask >> st) & 1) {
      const int x = (int)(fr.xdiag >> (NB * st)) & (NT - 1);
      std::vector<cd> stg(kTabA + kTabB);
      for (int t = 0; t < kTabA + kTabB; ++t) {
        const bool hi = t >= kTabA;
        const int ti = hi ? t - kTabA : t;
        const int j = ti ^ (hi ? x >> 6 : x & (kTabA - 1));
        const int zt = hi ? fr.zlast >> 6 : fr.zlast & 63;
        const bool neg = st == last && (__builtin_popcount(j & zt) & 1);
        stg[(hi ? kTabA : 0) + j] = neg ? -c.tab[st][t] : c.tab[st][t];
      }
      for (int y = 0; y < NT; ++y) ref[y] *= stg[y & (kTabA - 1)] * stg[kTabA + (y >> 6)];
    }
    if (st == n) break;
    for (int k : step_sites(c, st))
      for (int y = 0; y < NT; ++y)
        if (!((y >> k) & 1)) bfly(c.rx, fr.coef[st][k], ref[y], ref[y | (1 << k)]);
  }

  // the kernel's program on threads and registers
  Regs<cd> v;
  for (int t = 0; t < kThreads; ++t)
    for (int r = 0; r < kRegs; ++r) v(t, r) = psi[yof(kWfLayL2, t, r)];
  std::vector<int> owner(kSlots, -1);
  // wf_diag: the slot's register table staged (wf_reg_*), the thread's entry
  // fetched (wf_thr_*); L2 as layout 2, Q as layout 0 through its own map
  auto diag = [&](int lay, int st) {
    if (!((c.dmask >> st) & 1)) return;
    const int tl = lay == kWfLayL2 ? 2 : 0;
    const int x = (int)(fr.xdiag >> (NB * st)) & (NT - 1);
    std::vector<cd> reg(dtc::wf_reg_size(tl));
    for (int i = 0; i < dtc::wf_reg_size(tl); ++i) {
      const int j = i ^ dtc::wf_reg_xmask(tl, x);
      const bool neg = st == last && (__builtin_popcount(j & dtc::wf_reg_zmask(tl, fr.zlast)) & 1);
      const cd e = c.tab[st][dtc::wf_reg_base(tl) + i];
      reg[j] = neg ? -e : e;
    }
    for (int t = 0; t < kThreads; ++t) {
      const int yb = dtc::wf_t1_ybase(lay, t);
      cd e = c.tab[st][dtc::wf_thr_fetch(tl, yb, x)];
      if (st == last && dtc::wf_thr_neg(tl, yb, fr.zlast)) e = -e;
      for (int r = 0; r < kRegs; ++r) {
        // (the 0..6 table's entry first, as the model multiplies them)
        if (tl == 2) v(t, r) *= e * reg[((t >> 6) & 3) + 4 * r];
        else v(t, r) *= reg[(yb & 0x70) + r] * e;
      }
    }
  };
  auto kick_reg = [&](int q, double f) {
    for (int t = 0; t < kThreads; ++t)
      for (int r = 0; r < kRegs; ++r)
        if (!(r & (1 << q))) bfly(c.rx, f, v(t, r), v(t, r | (1 << q)));
  };
  auto kick_nib = [&](int nib, int st) {
    if (!(c.mask[st] & (0xFu << (4 * nib)))) return;
    for (int q = 0; q < 4; ++q) kick_reg(q, fr.coef[st][4 * nib + q]);
  };
  auto kick_pair = [&](int h, int st) {
    if (!(c.mask[st] & 0xF0u)) return;
    kick_reg(0, fr.coef[st][4 + 2 * h]);
    kick_reg(1, fr.coef[st][5 + 2 * h]);
  };
  int st = 0;
  do {
    diag(kWfLayL2, st);
    if (st < n) {
      kick_nib(2, st);
      t1_swap(v);
      kick_pair(0, st);
      if (!exchange(v, kWfLayL2s, kWfLayQs, owner, true)) return false;
      kick_pair(1, st);
      t1_swap(v);
      kick_nib(0, st);
      diag(kWfLayQ, st + 1);
      if (st + 1 < n) {
        kick_nib(0, st + 1);
        t1_swap(v);
        kick_pair(1, st + 1);
        if (!exchange(v, kWfLayQs, kWfLayL2s, owner, true)) return false;
        kick_pair(0, st + 1);
        t1_swap(v);
        kick_nib(2, st + 1);
      }
    }
    st += 2;
  } while (st <= n);
  if (n & 1)
    if (!exchange(v, kWfLayQ, kWfLayL2, owner, false)) return false;

  for (int t = 0; t < kThreads; ++t)
    for (int r = 0; r < kRegs; ++r) {
      const cd a = v(t, r), b = ref[yof(kWfLayL2, t, r)];
      CHECK(std::memcmp(&a, &b, sizeof(cd)) == 0, "program: index %d: %.17g%+.17gi, model %.17g%+.17gi",
            yof(kWfLayL2, t, r), a.real(), a.imag(), b.real(), b.imag());
    }
  return true;
}

bool check_program(long& n_cases) {
  for (int rx = 0; rx < 2; ++rx)
    for (int n_steps = 1; n_steps <= NS; ++n_steps)
      for (int trailing = 0; trailing < 2; ++trailing)
        for (int mk = 0; mk < 5; ++mk)
          for (int seed = 0; seed < 4; ++seed) {
            const int first = (seed >> 1) & 1;  // the diagonal before step 0
            std::mt19937_64 rng(1000003ull * seed + 7919 * mk + 131 * n_steps + 17 * trailing + rx);
            std::uniform_real_distribution<double> cf(-1.0, 1.0);
            Case c;
            c.rx = rx;
            c.n_steps = n_steps;
            c.out = seed & 1;
            c.dmask = trailing << n_steps;
            for (int st = 0; st < NS; ++st) {
              uint32_t m = 0xFFFu;
              // mk 1..3: the junction in steps (mk - 1, mk) only; mk 2 is the
              // steady pass's (steps 1 and 2); mk 4: random bits, which leave
              // out whole nibbles too
              if (mk >= 1 && mk <= 3 && st != mk - 1 && st != mk) m &= ~(1u << 11);
              if (mk == 4) {
                m &= (uint32_t)rng();
                if (rng() & 1) m &= ~(0xFu << (4 * (int)(rng() % 3)));
                m |= 1u << (int)(rng() % 12);
              }
              c.mask[st] = st < n_steps ? m : 0u;
              if (st < n_steps && (st || first)) c.dmask |= 1 << st;
              for (int k = 0; k < NB; ++k) {
                const bool on = (c.mask[st] >> k) & 1;
                c.var[st][k] = on ? (int)(rng() & 3) : 0;
                c.coef[st][k] = on ? cf(rng) : 0.0;
              }
            }
            for (int st = 0; st <= NS; ++st) c.tab[st] = make_tables(rng, c.out);
            if (!run_case(c, rng)) {
              std::printf("  (rx %d steps %d dmask %d masks %d seed %d)\n", rx, n_steps, c.dmask, mk, seed);
              return false;
            }
            ++n_cases;
          }
  return true;
}

}  // namespace

int main() {
  if (!check_indices()) return 1;
  long n_instr = 0, n_cases = 0;
  if (!check_banks(n_instr)) return 1;
  if (!check_table_reads()) return 1;
  if (!check_program(n_cases)) return 1;
  std::printf("wavefront t1 swap: ok (%ld LDS instructions conflict-free, %ld program cases bit-equal)\n",
              n_instr, n_cases);
  return 0;
}
