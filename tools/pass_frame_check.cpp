// pass_frame_check.cpp -- the program and the Pauli frame of the 12-bit K-D-K
// passes (csrc/dtc_pass_frame.h: pass_program, which pass_body reads at compile
// time, and frame12_walk, the code the prep kernel runs) on the CPU: a
// 4096-amplitude tile goes through one pass twice,
//   directly: every kicked bit's 2x2 matrix diag(1, sigma) S of its variant in
//             program order (pre-kick nibbles IO, 0, O; post-kick O, 0, IO), a
//             random diagonal between the two kick layers;
//   in frame form, as pass_body runs it: the form-B butterfly G(f^) with the
//             walk's coefficient for every bit of a kicked nibble; at each
//             re-layout site the tile index-permuted by mw[e] ^ mr[e] of the
//             re-layout e the site names (PassProgram::before / last, as the
//             kernel's sites do); at the diagonal point the sign of parity
//             (y & md) -- also in a pass without a diagonal, where the kernel
//             signs with the global factor -- and i^ph on the whole tile,
// and the two tiles must agree to 1e-12 (both scaled by the kicks' common
// 1 / sqrt(1 + coef^2), so the tile keeps norm 1).
// The dual pass's echo branch: the forward K-D-K's tile is copied after the
// pre-kick; the copy takes the Z flush of its own records (the forward's
// pre-kick with the echo chain's first layer as post-kick, no diagonal) as a
// sign there, its own X masks at the forward's post re-layouts, its own
// post-kick coefficients and power of i, and must equal post2 . pre applied
// directly.  (Its records' pre half -- coefficients and masks -- must be the
// forward's: the copy has been through the forward's.)
// Cases: RX and RY; nibble sets 1..7 (the kernel runs 6 and 7 in frame form);
// pre-only, post-only and both; with and without the diagonal; random variants
// and coefficients, some bits with the identity record (variant 0, coefficient
// 0: an inactive site of a kicked nibble).  Over the seeds every variant must
// occur on every kicked bit of every (kind, nibble set, half).
// Invariants per case: at most kT12Masks real re-layouts, and no mask beyond
// them; every site's (from, to) is its re-layout's; mw[e] has no bit in the
// register nibble of re-layout e's source layout, mr[e] none in its target's;
// the frame is the identity at the store.  (A pass without any re-layout -- the
// IO nibble alone, set 4 -- has nothing to flush X with, so pass_body could not
// run it in frame form, and does not.  The walk's bookkeeping is checked there
// all the same, with the X carried as the wavefront pass carries it: the
// diagonal read at index y ^ x, the tile stored at y ^ x, the frame left at the
// store X^x alone.)
//
// Host only: c++ -std=c++17 -I <csrc> tools/pass_frame_check.cpp (it may also
// be built with -fsanitize=address,undefined and run as it is).
#include <cmath>
#include <complex>
#include <cstdio>
#include <random>
#include <vector>

#include "dtc_pass_frame.h"

namespace {

using cd = std::complex<double>;
constexpr int NB = dtc::kPassBits, NT = 1 << NB;

struct Case {
  bool rx;
  int nibs;
  bool pre, post, diag;
  int var[2 * NB];
  double coef[2 * NB];
  int var2[2 * NB];  // the echo branch's records: pre as above, its own post
  double coef2[2 * NB];
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

void sign_flush(std::vector<cd>& v, int zm) {
  for (int y = 0; y < NT; ++y)
    if (__builtin_popcount(y & zm) & 1) v[y] = -v[y];
}

bool fail(const char* what) {
  std::printf("FAIL invariant: %s\n", what);
  return false;
}

// the walk's invariants for the program P
bool check_frame(const dtc::PassProgram& P, const dtc::Frame12& fr) {
  if (P.n_rl > dtc::kT12Masks) return fail("more than kT12Masks real re-layouts");
  for (int e = 0; e < dtc::kT12Masks; ++e) {
    if (e >= P.n_rl) {
      if (fr.mw[e] | fr.mr[e]) return fail("a mask beyond the pass's re-layouts");
      continue;
    }
    if ((fr.mw[e] | fr.mr[e]) & ~(NT - 1)) return fail("a mask bit outside the tile");
    if ((fr.mw[e] >> (4 * P.rl[e].from)) & 15) return fail("mw on its source layout's registers");
    if ((fr.mr[e] >> (4 * P.rl[e].to)) & 15) return fail("mr on its target layout's registers");
  }
  if (fr.end.z) return fail("Z left in the frame at the store");
  if (P.n_rl > 0 && fr.end.x) return fail("X left in the frame at the store");
  return true;
}

// The pass in frame form, in pass_body's order.  fr2 (the dual pass): the echo
// branch's records; its tile comes back in `echo`.
bool run_frame(const Case& c, const dtc::PassProgram& P, const dtc::Frame12& fr,
               const std::vector<cd>& dg, std::vector<cd>& v, const dtc::Frame12* fr2,
               std::vector<cd>* echo) {
  const bool n0 = c.nibs & 1, nIO = (c.nibs >> P.IO) & 1, nO = (c.nibs >> P.O) & 1;
  std::vector<cd> tmp(NT);
  int lay = P.IO;
  bool ok = true, co = false;  // co: the echo tile rides along
  auto permute = [&](std::vector<cd>& t, int m) {
    for (int y = 0; y < NT; ++y) tmp[y] = t[y ^ m];
    t.swap(tmp);
  };
  // a re-layout site: to layout `to`, named e by the plan
  auto relayout = [&](int to, int e) {
    if (!P.names(e, lay, to)) ok = fail("a site's re-layout is not the plan's");
    if (lay != to && ok) {
      permute(v, fr.mw[e] ^ fr.mr[e]);
      if (co) permute(*echo, fr2->mw[e] ^ fr2->mr[e]);
    }
    lay = to;
  };
  auto nibble = [&](int half, int nib) {
    for (int q = 0; q < 4; ++q) {
      const int i = half * NB + 4 * nib + q;
      kick_g(v, c.rx, 4 * nib + q, fr.coef[i]);
      if (co) kick_g(*echo, c.rx, 4 * nib + q, fr2->coef[i]);
    }
  };
  if (c.pre) {
    if (nIO) nibble(0, P.IO);
    if (n0) relayout(0, P.before(0, 0)), nibble(0, 0);
    if (nO) {
      if (lay != P.k0) ok = fail("k0 is not the layout behind the nibble-0 round");
      relayout(P.O, P.before(0, P.O)), nibble(0, P.O);
    }
  }
  if (lay != P.d_lay) ok = fail("d_lay is not where the pre-kick ends");
  if (fr2) {
    *echo = v;
    sign_flush(*echo, fr2->md);
    co = true;
  }
  sign_flush(v, fr.md);
  // (the frame's X here: none, but for the pass without re-layouts)
  int xd = 0;
  if (P.n_rl == 0 && c.pre)
    for (int k = 0; k < NB; ++k)
      if ((c.nibs >> (k >> 2)) & 1) xd |= dtc::frame_form_a(c.var[k]) << k;
  if (c.diag)
    for (int y = 0; y < NT; ++y) v[y] *= dg[y ^ xd];
  if (c.post) {
    if (nO) relayout(P.O, P.before(1, P.O)), nibble(1, P.O);
    if (lay != P.pO) ok = fail("pO");
    if (n0) relayout(0, P.before(1, 0)), nibble(1, 0);
    if (lay != P.p0) ok = fail("p0");
    if (nIO) relayout(P.IO, P.before(1, P.IO)), nibble(1, P.IO);
    if (lay != P.pIO) ok = fail("pIO");
  }
  relayout(P.IO, P.last());
  const cd ip[4] = {cd(1, 0), cd(0, 1), cd(-1, 0), cd(0, -1)};
  for (cd& a : v) a *= ip[fr.ph];
  if (co)
    for (cd& a : *echo) a *= ip[fr2->ph];
  return ok;
}

// one layer's kicks applied directly, nibbles in the order `ord`
double direct_layer(const Case& c, std::vector<cd>& v, const int* var, const double* coef,
                    int half, const int (&ord)[3]) {
  double w = 1.0;
  for (int nib : ord) {
    if (!((c.nibs >> nib) & 1)) continue;
    for (int k = 4 * nib; k < 4 * nib + 4; ++k) {
      kick_direct(v, c.rx, k, var[half * NB + k], coef[half * NB + k]);
      w /= std::sqrt(1.0 + coef[half * NB + k] * coef[half * NB + k]);
    }
  }
  return w;
}

double max_err(const std::vector<cd>& got, const std::vector<cd>& ref, double w, int x) {
  double err = 0.0;
  for (int y = 0; y < NT; ++y) {
    const double e = std::abs(w * (got[y] - ref[y ^ x]));
    if (!(e <= err)) err = e;  // (a NaN stays)
  }
  return err;
}

// worst error of the case (of both tiles with `dual`), < 0: an invariant failed
double run_case(const Case& c, bool dual, std::mt19937_64& rng) {
  std::normal_distribution<double> nd;
  std::uniform_real_distribution<double> ang(-M_PI, M_PI);
  std::vector<cd> psi(NT), dg(NT);
  double nrm = 0.0;
  for (cd& a : psi) a = cd(nd(rng), nd(rng)), nrm += std::norm(a);
  for (cd& a : psi) a /= std::sqrt(nrm);
  for (cd& a : dg) a = std::polar(1.0, ang(rng));

  const dtc::PassProgram P = dtc::pass_program(c.nibs, c.pre, c.post);
  const int pre_ord[3] = {P.IO, 0, P.O}, post_ord[3] = {P.O, 0, P.IO};
  std::vector<cd> ref = psi, ref2;
  double w = 1.0, w2 = 1.0;
  if (c.pre) w *= direct_layer(c, ref, c.var, c.coef, 0, pre_ord);
  if (dual) {
    ref2 = ref;
    w2 = w * direct_layer(c, ref2, c.var2, c.coef2, 1, post_ord);
  }
  if (c.diag)
    for (int y = 0; y < NT; ++y) ref[y] *= dg[y];
  if (c.post) w *= direct_layer(c, ref, c.var, c.coef, 1, post_ord);

  dtc::Frame12 fr, fr2;
  dtc::frame12_walk(c.rx, c.nibs, c.pre, c.post, c.var, c.coef, fr);
  if (!check_frame(P, fr)) return -1.0;
  if (dual) {
    dtc::frame12_walk(c.rx, c.nibs, c.pre, c.post, c.var2, c.coef2, fr2);
    if (!check_frame(P, fr2)) return -1.0;
    // the copy has been through the forward's pre-kick
    int n_pre = 0;
    for (int i = 0; i < P.n_ev && P.ev[i].type != dtc::kEvDiag; ++i)
      if (P.ev[i].type == dtc::kEvRelayout) ++n_pre;
    for (int e = 0; e < n_pre; ++e)
      if (fr.mw[e] != fr2.mw[e] || fr.mr[e] != fr2.mr[e])
        return fail("the echo branch's pre-kick masks differ from the forward's"), -1.0;
    for (int k = 0; k < NB; ++k)
      if (fr.coef[k] != fr2.coef[k])
        return fail("the echo branch's pre-kick coefficients differ from the forward's"), -1.0;
  }
  std::vector<cd> got = psi, got2;
  if (!run_frame(c, P, fr, dg, got, dual ? &fr2 : nullptr, &got2)) return -1.0;
  double err = max_err(got, ref, w, fr.end.x);
  if (dual) {
    const double e2 = max_err(got2, ref2, w2, fr2.end.x);
    if (!(e2 <= err)) err = e2;
  }
  return err;
}

}  // namespace

int main() {
  constexpr int kSeeds = 16;
  static int cover[2][8][2][NB];  // variants seen per (kind, nibble set, half, bit)
  double worst = 0.0;
  long n_cases = 0;
  for (int rx = 0; rx < 2; ++rx)
    for (int nibs = 1; nibs < 8; ++nibs)
      // modes 0..5: pre-only, post-only, both, each without / with the diagonal;
      // 6: the dual pass (both, with the diagonal, and its echo branch)
      for (int mode = 0; mode < 7; ++mode)
        for (int seed = 0; seed < kSeeds; ++seed) {
          std::mt19937_64 rng(1000003ull * seed + 7919 * mode + 131 * nibs + rx);
          std::uniform_real_distribution<double> cf(-1.0, 1.0);
          const bool dual = mode == 6;
          Case c;
          c.rx = rx;
          c.nibs = nibs;
          c.pre = dual || mode % 3 != 1;
          c.post = dual || mode % 3 != 0;
          c.diag = dual || mode >= 3;
          for (int i = 0; i < 2 * NB; ++i) {
            const int half = i / NB, k = i % NB;
            const bool on = ((nibs >> (k >> 2)) & 1) && (half ? c.post : c.pre);
            const bool ident = on && rng() % 16 == 0;  // an inactive site's record
            c.var[i] = (on && !ident) ? (int)(rng() & 3) : 0;
            c.coef[i] = (on && !ident) ? cf(rng) : 0.0;
            if (on) cover[rx][nibs][half][k] |= 1 << c.var[i];
            const bool own = dual && half == 1;
            c.var2[i] = own ? (int)(rng() & 3) : c.var[i];
            c.coef2[i] = own ? cf(rng) : c.coef[i];
          }
          const double err = run_case(c, dual, rng);
          ++n_cases;
          if (!(err >= 0.0 && err < 1e-12)) {
            std::printf("FAIL rx %d nibs %d mode %d seed %d: %.3e\n", rx, nibs, mode, seed, err);
            return 1;
          }
          if (err > worst) worst = err;
        }
  for (int rx = 0; rx < 2; ++rx)
    for (int nibs = 1; nibs < 8; ++nibs)
      for (int half = 0; half < 2; ++half)
        for (int k = 0; k < NB; ++k)
          if (((nibs >> (k >> 2)) & 1) && cover[rx][nibs][half][k] != 15) {
            std::printf("FAIL coverage: rx %d nibs %d half %d bit %d saw variants 0x%x\n", rx, nibs,
                        half, k, cover[rx][nibs][half][k]);
            return 1;
          }
  std::printf("pass frames: ok (%ld cases, worst %.3e)\n", n_cases, worst);
  return 0;
}
