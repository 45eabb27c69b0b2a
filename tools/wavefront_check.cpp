// Stand-alone check of the wavefront planner (csrc/dtc_wavefront.h), host only:
//
//   g++ -std=c++17 -O1 -I <pkg>/csrc tools/wavefront_check.cpp -o wavefront_check
//   ./wavefront_check                 exhaustive check of the L = 20 tiles, exit 0 / 1
//   ./wavefront_check --table         the same, and the launch counts per span
//   ./wavefront_check --dump L split y low_ahead span cap  n_tiles {n_cols s0 n_sites}...
//                                     one plan as text (tests/test_wavefront_planner.py)
//
// (it may also be built with -fsanitize=address,undefined and run as it is).
// The checker replays a plan event by event with its own bookkeeping; it shares
// no logic with the planner beyond the data structures.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "dtc_wavefront.h"

using namespace dtc::wf;

static std::string g_err;

static bool bad(const char* what, int pass, int step, int site, int layer) {
  char buf[256];
  std::snprintf(buf, sizeof buf, "%s (pass %d step %d site %d layer %d)", what, pass, step, site,
                layer);
  g_err = buf;
  return false;
}

static bool tile_has(const Tile& t, int s) {
  for (int k = 0; k < t.n_bits; ++k)
    if (t.site[k] == s) return true;
  return false;
}

// Every (site, layer) kicked exactly once and in order, every factor applied
// exactly once between the right kicks, every stencil dependency met, the
// target reached, the pass shapes within their limits.
static bool verify(const Problem& p, const std::vector<Pass>& plan) {
  const int L = p.L;
  std::vector<int> kicked(p.f0), fld(L, p.d0), bnd(L > 1 ? L - 1 : 0, p.d0);
  for (size_t pi = 0; pi < plan.size(); ++pi) {
    const Pass& ps = plan[pi];
    if (ps.tile < 0 || ps.tile >= (int)p.tiles.size()) return bad("tile index", pi, -1, -1, -1);
    const Tile& t = p.tiles[ps.tile];
    if (ps.steps.empty()) return bad("empty pass", pi, -1, -1, -1);
    int kick_steps = 0;
    for (size_t si = 0; si < ps.steps.size(); ++si) {
      const Step& sp = ps.steps[si];
      if (!sp.kick_mask && sp.factors.empty()) return bad("empty step", pi, si, -1, -1);
      if (!sp.kick_mask && si + 1 != ps.steps.size())
        return bad("kick-less step not last", pi, si, -1, -1);
      if (sp.kick_mask >> t.n_bits) return bad("mask beyond tile", pi, si, -1, -1);
      kick_steps += sp.kick_mask != 0;
      // factors first, on the state before this step's kicks
      for (const Factor& f : sp.factors) {
        const int s = f.site, m = f.layer;
        if (!f.bond) {
          if (s < 0 || s >= L) return bad("field site", pi, si, s, m);
          if (!tile_has(t, s)) return bad("field outside tile", pi, si, s, m);
          if (fld[s] != m - 1) return bad("field out of order / repeated", pi, si, s, m);
          if (kicked[s] != m - 1) return bad("field not between k(m-1), k(m)", pi, si, s, m);
          fld[s] = m;
        } else {
          if (s < 0 || s + 1 >= L) return bad("bond site", pi, si, s, m);
          if (!tile_has(t, s) && !tile_has(t, s + 1)) return bad("bond outside tile", pi, si, s, m);
          if (bnd[s] != m - 1) return bad("bond out of order / repeated", pi, si, s, m);
          if (kicked[s] != m - 1 || kicked[s + 1] != m - 1)
            return bad("bond not between k(m-1), k(m)", pi, si, s, m);
          bnd[s] = m;
        }
      }
      // then the kicks, all against the frontier before the step
      const std::vector<int> before(kicked);
      for (int k = 0; k < t.n_bits; ++k) {
        if (!((sp.kick_mask >> k) & 1u)) continue;
        const int s = t.site[k], m = sp.layer[k];
        if (s < 0) return bad("kick on a column bit", pi, si, s, m);
        if (before[s] != m - 1) return bad("kick out of order / repeated", pi, si, s, m);
        if (m > p.f1[s]) return bad("kick beyond target", pi, si, s, m);
        if (fld[s] != m) return bad("kick without its field", pi, si, s, m);
        if (s > 0 && (bnd[s - 1] != m || before[s - 1] < m - 1))
          return bad("kick before left stencil", pi, si, s, m);
        if (s + 1 < L && (bnd[s] != m || before[s + 1] < m - 1))
          return bad("kick before right stencil", pi, si, s, m);
        kicked[s] = m;
      }
    }
    if (kick_steps > p.cap) return bad("more kick steps than the cap", pi, -1, -1, -1);
  }
  for (int s = 0; s < L; ++s) {
    if (kicked[s] != p.f1[s]) return bad("target frontier missed", -1, -1, s, kicked[s]);
    if (fld[s] != p.d1) return bad("target field level missed", -1, -1, s, fld[s]);
  }
  for (int b = 0; b + 1 < L; ++b)
    if (bnd[b] != p.d1) return bad("target bond level missed", -1, -1, b, bnd[b]);
  if ((int)plan.size() > p.max_passes) return bad("more launches than plain", -1, -1, -1, -1);
  return true;
}

static bool same(const std::vector<Pass>& a, const std::vector<Pass>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i) {
    if (a[i].tile != b[i].tile || a[i].steps.size() != b[i].steps.size()) return false;
    for (size_t j = 0; j < a[i].steps.size(); ++j) {
      const Step &x = a[i].steps[j], &y = b[i].steps[j];
      if (x.kick_mask != y.kick_mask || x.factors.size() != y.factors.size()) return false;
      if (std::memcmp(x.layer, y.layer, sizeof x.layer)) return false;
      for (size_t k = 0; k < x.factors.size(); ++k)
        if (x.factors[k].bond != y.factors[k].bond || x.factors[k].site != y.factors[k].site ||
            x.factors[k].layer != y.factors[k].layer)
          return false;
    }
  }
  return true;
}

static int check_all(bool table) {
  int fails = 0;
  for (int cap = 2; cap <= 4; ++cap) {
    for (int low_ahead = 0; low_ahead <= 1; ++low_ahead) {
      for (int y = 1; y <= 2; ++y) {
        int prev = 0;
        for (int span = 3; span <= 23; ++span) {
          Problem p = plain_span(20, 12, y, low_ahead != 0, span);
          p.tiles = {make_tile(0, 0, 12), make_tile(3, 11, 9)};
          p.cap = cap;
          std::vector<Pass> plan, again;
          const bool ok = dtc::wf::plan(p, plan);
          if (!ok) {
            std::printf("FAIL cap %d low_ahead %d y %d span %d: no plan\n", cap, low_ahead, y, span);
            ++fails;
            continue;
          }
          if (!verify(p, plan)) {
            std::printf("FAIL cap %d low_ahead %d y %d span %d: %s\n", cap, low_ahead, y, span,
                        g_err.c_str());
            ++fails;
          }
          dtc::wf::plan(p, again);
          if (!same(plan, again)) {
            std::printf("FAIL cap %d low_ahead %d y %d span %d: not deterministic\n", cap,
                        low_ahead, y, span);
            ++fails;
          }
          if ((int)plan.size() < prev) {
            std::printf("FAIL cap %d low_ahead %d y %d span %d: %d launches after %d\n", cap,
                        low_ahead, y, span, (int)plan.size(), prev);
            ++fails;
          }
          prev = (int)plan.size();
          if (table && y == 1) {
            int kicks = 0, max_kicks = 0;
            for (const Pass& ps : plan) {
              int n = 0;
              for (const Step& sp : ps.steps) n += __builtin_popcount(sp.kick_mask);
              kicks += n;
              if (n > max_kicks) max_kicks = n;
            }
            std::printf("cap %d %s span %2d: %2d launches (plain %2d), %3d site kicks, "
                        "%2d in the largest pass\n",
                        cap, low_ahead ? "A ahead" : "B ahead", span, (int)plan.size(), span,
                        kicks, max_kicks);
          }
        }
      }
    }
  }
  // a cap of 1 can do no better than the plain schedule, and a limit below
  // what the plan needs must be refused, not exceeded
  {
    Problem p = plain_span(20, 12, 1, true, 8);
    p.tiles = {make_tile(0, 0, 12), make_tile(3, 11, 9)};
    std::vector<Pass> plan;
    p.max_passes = 2;
    if (dtc::wf::plan(p, plan) || !plan.empty()) {
      std::printf("FAIL: a plan over the launch limit was returned\n");
      ++fails;
    }
    // tiles without a shared site still work, one period per pass
    p.tiles = {make_tile(0, 0, 12), make_tile(4, 12, 8)};
    p.max_passes = 8;
    if (!dtc::wf::plan(p, plan) || !verify(p, plan)) {
      std::printf("FAIL: disjoint tiles: %s\n", g_err.c_str());
      ++fails;
    }
    // tiles that do not cover the chain cannot plan
    p.tiles = {make_tile(0, 0, 12)};
    if (dtc::wf::plan(p, plan)) {
      std::printf("FAIL: a plan for tiles that miss sites\n");
      ++fails;
    }
  }
  std::printf(fails ? "wavefront planner: %d failures\n" : "wavefront planner: ok\n", fails);
  return fails ? 1 : 0;
}

static int dump(int argc, char** argv) {
  // L split y low_ahead span cap n_tiles {n_cols s0 n_sites}...
  if (argc < 7) return 2;
  const int L = std::atoi(argv[0]), split = std::atoi(argv[1]), y = std::atoi(argv[2]);
  const int low_ahead = std::atoi(argv[3]), span = std::atoi(argv[4]), cap = std::atoi(argv[5]);
  const int nt = std::atoi(argv[6]);
  if (nt < 1 || argc != 7 + 3 * nt || L < 1 || L > 64) return 2;
  Problem p = plain_span(L, split, y, low_ahead != 0, span);
  p.cap = cap;
  for (int i = 0; i < nt; ++i) {
    const int nc = std::atoi(argv[7 + 3 * i]), s0 = std::atoi(argv[8 + 3 * i]);
    const int ns = std::atoi(argv[9 + 3 * i]);
    if (nc < 0 || ns < 1 || nc + ns > kMaxTileBits || s0 < 0 || s0 + ns > L) return 2;
    p.tiles.push_back(make_tile(nc, s0, ns));
  }
  std::vector<Pass> plan;
  if (!dtc::wf::plan(p, plan)) {
    std::printf("noplan\n");
    return 0;
  }
  if (!verify(p, plan)) {
    std::printf("invalid %s\n", g_err.c_str());
    return 1;
  }
  std::printf("frontier");
  for (int s = 0; s < L; ++s) std::printf(" %d", p.f0[s]);
  std::printf("\ntarget");
  for (int s = 0; s < L; ++s) std::printf(" %d", p.f1[s]);
  std::printf("\ndiag %d %d\n", p.d0, p.d1);
  for (const Pass& ps : plan) {
    std::printf("pass %d\n", ps.tile);
    for (const Step& sp : ps.steps) {
      std::printf("step %x\n", sp.kick_mask);
      for (const Factor& f : sp.factors)
        std::printf("%s %d %d\n", f.bond ? "b" : "f", (int)f.site, (int)f.layer);
      for (int k = 0; k < p.tiles[ps.tile].n_bits; ++k)
        if ((sp.kick_mask >> k) & 1u)
          std::printf("k %d %d\n", p.tiles[ps.tile].site[k], (int)sp.layer[k]);
    }
  }
  std::printf("end\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !std::strcmp(argv[1], "--dump")) return dump(argc - 2, argv + 2);
  return check_all(argc >= 2 && !std::strcmp(argv[1], "--table"));
}
