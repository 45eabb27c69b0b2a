// Wavefront planner (host only): the order in which overlapping tiles advance
// a chain of Floquet layers by more than one period per pass over the state.
//
// A chain is X_0 D_1 X_1 D_2 X_2 ...: kick layer m (single-site kicks k(s, m))
// follows the diagonal D_m, a product of commuting factors -- a field factor
// per site and a bond factor per pair (s, s+1) of the open chain.  The result
// needs only the three-point stencil order:
//   field(s, m)  after k(s, m-1),              before k(s, m);
//   bond(s, m)   after k(s, m-1), k(s+1, m-1), before k(s, m), k(s+1, m).
// Any schedule that keeps it is the same operator, so a tile may lift its
// sites by several layers in one pass as long as the sites next to them -- in
// the tile or not -- are far enough along.  Two tiles that share a junction
// site (L = 20: sites 0..11 and sites 11..19) reach a steady state in which
// each pass lifts its own sites by `cap` layers and the junction by cap / 2:
// two passes per `cap` periods instead of one pass per period.
//
// The planner keeps a frontier f(s), the last kick layer applied per site, and
// the level of every diagonal factor.  A pass over a tile is a list of
// layer-steps; a step names the tile bits that take their next kick and the
// factors applied just before those kicks.  A factor of layer m is applied
// exactly once, in the step in which the first of its sites takes k(m); a
// factor none of whose sites takes k(m) before the target (the target's own
// closing diagonal) goes into a trailing kick-less step of the pass that
// brings its sites to layer m-1.  A bond to a site outside the tile is a
// constant of the workgroup: a sign on the in-tile site's angle.
//
// Sites that belong to the same tiles form a block; a block moves only as a
// whole, so the frontier stays piecewise constant (few distinct factor sets).
#pragma once

#include <cstdint>
#include <vector>

namespace dtc {
namespace wf {

constexpr int kMaxTileBits = 12;

// Tile bit k holds site `site[k]`, or a column bit (an index bit that is not
// kicked by this tile) when site[k] < 0.
struct Tile {
  int n_bits = 0;
  int site[kMaxTileBits] = {};
};

inline Tile make_tile(int n_cols, int s0, int n_sites) {
  Tile t;
  t.n_bits = n_cols + n_sites;
  for (int k = 0; k < n_cols; ++k) t.site[k] = -1;
  for (int k = 0; k < n_sites; ++k) t.site[n_cols + k] = s0 + k;
  return t;
}

struct Factor {
  int8_t bond;    // 0: field of `site`; 1: bond (site, site + 1)
  int8_t site;
  int16_t layer;
};

struct Step {
  uint32_t kick_mask = 0;                // tile bits that take their next kick
  int16_t layer[kMaxTileBits] = {};      // the layer each of them takes
  std::vector<Factor> factors;           // applied before the step's kicks
};

struct Pass {
  int tile = 0;
  std::vector<Step> steps;               // a trailing step may have no kicks
};

struct Problem {
  int L = 0;
  std::vector<int> f0;                   // start frontier per site
  int d0 = 0;                            // every factor applied through layer d0
  std::vector<int> f1;                   // target frontier per site
  int d1 = 0;                            // every factor applied through layer d1
  std::vector<Tile> tiles;
  int cap = 4;                           // kick steps per pass at most
  int max_passes = 1 << 30;              // the plain schedule's launches for the span
};

namespace detail {

struct State {
  std::vector<int> f, fld, bnd;  // frontier, field level per site, bond level per (s, s+1)
};

inline bool in_tile(const Tile& t, int s) {
  for (int k = 0; k < t.n_bits; ++k)
    if (t.site[k] == s) return true;
  return false;
}

inline bool eligible(const Problem& p, const State& st, int s) {
  if (st.f[s] >= p.f1[s]) return false;
  if (s > 0 && st.f[s - 1] < st.f[s]) return false;
  if (s + 1 < p.L && st.f[s + 1] < st.f[s]) return false;
  return true;
}

// One pass over tile ti from state st; false if it would do nothing.
inline bool build_pass(const Problem& p, const std::vector<int>& block, int ti, State& st,
                       Pass& out) {
  const Tile& t = p.tiles[ti];
  out.tile = ti;
  out.steps.clear();
  const int L = p.L;
  for (int n = 0; n < p.cap; ++n) {
    // the sites that move: whole blocks (of one frontier and one target) only
    std::vector<char> mv(L, 0);
    for (int k = 0; k < t.n_bits; ++k)
      if (t.site[k] >= 0) mv[t.site[k]] = eligible(p, st, t.site[k]);
    for (int s = 0; s < L; ++s) {
      if (!mv[s]) continue;
      bool whole = true, uniform = true;
      for (int q = 0; q < L; ++q) {
        if (block[q] != block[s]) continue;
        uniform = uniform && st.f[q] == st.f[s] && p.f1[q] == p.f1[s];
        whole = whole && in_tile(t, q) && eligible(p, st, q);
      }
      if (uniform && !whole) mv[s] = 0;
    }
    Step sp;
    for (int k = 0; k < t.n_bits; ++k) {
      const int s = t.site[k];
      if (s < 0 || !mv[s]) continue;
      sp.kick_mask |= 1u << k;
      sp.layer[k] = (int16_t)(st.f[s] + 1);
    }
    if (!sp.kick_mask) break;
    // the factors of the kicked sites' next layers that are still pending
    for (int s = 0; s < L; ++s) {
      if (!mv[s]) continue;
      const int m = st.f[s] + 1;
      if (st.fld[s] == m - 1) {
        sp.factors.push_back(Factor{0, (int8_t)s, (int16_t)m});
        st.fld[s] = m;
      }
      for (int b = s - 1; b <= s; ++b) {
        if (b < 0 || b + 1 >= L) continue;
        if (st.bnd[b] == m - 1) {
          sp.factors.push_back(Factor{1, (int8_t)b, (int16_t)m});
          st.bnd[b] = m;
        }
      }
    }
    for (int s = 0; s < L; ++s) st.f[s] += mv[s];
    out.steps.push_back(sp);
  }
  // trailing step: the target's closing factors whose sites never take that
  // layer's kick, once their sites are at the layer before it
  Step tr;
  for (int s = 0; s < L; ++s) {
    const int m = st.fld[s] + 1;
    if (in_tile(t, s) && m <= p.d1 && p.f1[s] == m - 1 && st.f[s] == m - 1) {
      tr.factors.push_back(Factor{0, (int8_t)s, (int16_t)m});
      st.fld[s] = m;
    }
  }
  for (int b = 0; b + 1 < L; ++b) {
    const int m = st.bnd[b] + 1;
    if ((in_tile(t, b) || in_tile(t, b + 1)) && m <= p.d1 && p.f1[b] == m - 1 &&
        p.f1[b + 1] == m - 1 && st.f[b] == m - 1 && st.f[b + 1] == m - 1) {
      tr.factors.push_back(Factor{1, (int8_t)b, (int16_t)m});
      st.bnd[b] = m;
    }
  }
  if (!tr.factors.empty()) out.steps.push_back(tr);
  return !out.steps.empty();
}

inline bool done(const Problem& p, const State& st) {
  for (int s = 0; s < p.L; ++s)
    if (st.f[s] != p.f1[s] || st.fld[s] != p.d1) return false;
  for (int b = 0; b + 1 < p.L; ++b)
    if (st.bnd[b] != p.d1) return false;
  return true;
}

inline bool plan_from(const Problem& p, const std::vector<int>& block, int t0,
                      std::vector<Pass>& out) {
  State st{p.f0, std::vector<int>(p.L, p.d0), std::vector<int>(p.L > 1 ? p.L - 1 : 0, p.d0)};
  out.clear();
  const int nt = (int)p.tiles.size();
  int idle = 0;
  for (int ti = t0; !done(p, st); ti = (ti + 1) % nt) {
    Pass ps;
    if (build_pass(p, block, ti, st, ps)) {
      out.push_back(ps);
      idle = 0;
      if ((int)out.size() > p.max_passes) return false;
    } else if (++idle >= nt) {
      return false;  // no tile can move: the tiles do not cover the span
    }
  }
  return true;
}

}  // namespace detail

// Plan the passes from (f0, d0) to (f1, d1).  Deterministic: the tiles take
// turns, and of the possible first tiles the one with the fewest passes wins
// (the lowest index on a tie).  Returns false, and leaves `out` empty, when the
// problem is malformed, the tiles cannot reach the target, or the plan would
// take more than max_passes launches -- the caller then keeps its own schedule.
inline bool plan(const Problem& p, std::vector<Pass>& out) {
  out.clear();
  const int L = p.L;
  if (L < 1 || L > 64 || (int)p.f0.size() != L || (int)p.f1.size() != L || p.cap < 1 ||
      p.tiles.empty() || p.d1 < p.d0)
    return false;
  for (int s = 0; s < L; ++s) {
    // a start and a target that a plain schedule produces: the kicks at the
    // closed diagonal's layer or the one before, no kick beyond its layer
    if (p.f0[s] < 0 || (p.f0[s] != p.d0 && p.f0[s] != p.d0 - 1)) return false;
    if (p.f1[s] != p.d1 && p.f1[s] != p.d1 - 1) return false;
    if (p.f1[s] < p.f0[s]) return false;
  }
  for (const Tile& t : p.tiles) {
    if (t.n_bits < 1 || t.n_bits > kMaxTileBits) return false;
    for (int k = 0; k < t.n_bits; ++k)
      if (t.site[k] >= L) return false;
  }
  // blocks: runs of sites that belong to the same tiles
  std::vector<int> block(L, 0);
  std::vector<uint64_t> sig(L, 0);
  for (size_t ti = 0; ti < p.tiles.size() && ti < 64; ++ti)
    for (int s = 0; s < L; ++s)
      if (detail::in_tile(p.tiles[ti], s)) sig[s] |= 1ull << ti;
  for (int s = 1; s < L; ++s) block[s] = block[s - 1] + (sig[s] != sig[s - 1]);

  std::vector<Pass> best, cur;
  bool have = false;
  for (int t0 = 0; t0 < (int)p.tiles.size(); ++t0) {
    if (!detail::plan_from(p, block, t0, cur)) continue;
    if (!have || cur.size() < best.size()) {
      best = cur;
      have = true;
    }
  }
  if (!have) return false;
  out = best;
  return true;
}

// The frontiers of a run of `span` plain K-D-K passes that alternate between
// the site groups [0, split) and [split, L), entered with every diagonal
// through layer y applied, one group's kicks at y and the other's at y - 1
// (`low_ahead`: the low group is the one at y).  Each plain pass lifts the
// group that is behind by two layers and closes one diagonal.
inline Problem plain_span(int L, int split, int y, bool low_ahead, int span) {
  Problem p;
  p.L = L;
  p.d0 = y;
  p.d1 = y + span;
  p.f0.resize(L);
  p.f1.resize(L);
  // the group that moves last ends ahead: the one behind at entry if span is odd
  const bool low_ahead_end = (span % 2) ? !low_ahead : low_ahead;
  for (int s = 0; s < L; ++s) {
    const bool low = s < split;
    p.f0[s] = (low == low_ahead) ? y : y - 1;
    p.f1[s] = (low == low_ahead_end) ? y + span : y + span - 1;
  }
  p.max_passes = span;
  return p;
}

}  // namespace wf
}  // namespace dtc
