// dtc_pass_frame.h -- the program of a 12-bit K-D-K pass and its Pauli frame,
// host and device.  One description (pass_program) that the pass kernels read
// at compile time (dtc_kernels.hip, RoundPlan / pass_body), the prep kernel per
// state (frame12_records -> frame12_walk) and the engine on the host
// (launch_pass_spec); tools/pass_frame_check.cpp runs the same code on the CPU
// against the direct 2x2 products.
//
// The program: pre-kick nibbles IO -> 0 -> O with a re-layout before each but
// the first, the diagonal in layout d_lay, post-kick nibbles O -> 0 -> IO, the
// store from layout IO; a re-layout is skipped where the layout does not change.
//
// The frame: a pass in frame form runs one butterfly for every kick, the
// form-B one G(f) (RX: f I + i X; RY: f I + i Y).  The other forms become
// Paulis: form A is A(beta) = -i X G(-beta) (RX) or X Z G(-beta) (RY), sigma =
// -1 is a Z after the kick.  The true tile is i^ph X^x Z^z (the computed tile);
// a kick Z^n X^a G(g) on tile bit k runs as G(+-g) (G past the frame: RX flips
// g with Z_k, RY with X_k xor Z_k) and the frame takes Z^n X^a.
#pragma once
#include <stdint.h>

// (no other header: the CPU check compiles this file with a plain host compiler)
#ifdef __HIPCC__
#define DTC_PF_HD __host__ __device__
#else
#define DTC_PF_HD
#endif

namespace dtc {

// Load/store register layout of a pass over the register nibbles `nibs`
// (bit n = nibble n holds active sites): 1 (threads = tile bits 0..3, 8..11:
// 256-B row segments per 16 lanes) for the nibble sets in DTC_IO1_NIBS, else 2
// (threads = tile bits 0..7).  Same-box A/B (profiles/r1s_io_ab.json): the
// 12-site low group of C2 runs 1.60 -> 1.56 ms from layout 1.
#ifndef DTC_IO1_NIBS
#define DTC_IO1_NIBS (1 << 7)
#endif
constexpr int io_layout(int nibs) { return ((DTC_IO1_NIBS >> nibs) & 1) ? 1 : 2; }

static constexpr int kPassBits = 12;  // kTileBits
// the nibble set of a tile's active-bit mask (PassKick / PassArgs act)
constexpr int act_nibs(int act) {
  return ((act & 0xF) ? 1 : 0) | ((act & 0xF0) ? 2 : 0) | ((act & 0xF00) ? 4 : 0);
}
// the real re-layouts of any pass: one X-mask word each in the total record
// (dtc_kernels.h, kT12MaskX0 ..; static_assert below)
static constexpr int kT12Masks = 4;

enum PassEventType { kEvKick = 0, kEvRelayout = 1, kEvDiag = 2 };
static constexpr int kPassMaxEvents = 6 + kT12Masks + 1;  // kicks, re-layouts, the diagonal
struct PassEvent {
  int type;
  int arg;  // kEvKick: 4 half + nibble; kEvRelayout: its index e
};
struct PassRelayout {
  int from, to;
};
struct PassProgram {
  // IO = the load/store layout, O = 3 - IO the other high nibble; the diagonal's
  // layout (where the pre-kick ends); k0: the layout behind the pre-kick's
  // nibble-0 round; pO, p0, pIO: behind the post-kick's three rounds
  int IO, O, d_lay, k0, pO, p0, pIO;
  int n_rl;  // the real re-layouts, in program order
  PassRelayout rl[kT12Masks];
  int n_ev;  // kicks, re-layouts, the diagonal point (present in every pass)
  PassEvent ev[kPassMaxEvents];

  // the real re-layout right before the kick of `nib` in `half`, -1: none (the
  // nibble is not kicked, or the tile is in its layout already)
  constexpr int before(int half, int nib) const {
    for (int i = 1; i < n_ev; ++i)
      if (ev[i].type == kEvKick && ev[i].arg == 4 * half + nib)
        return ev[i - 1].type == kEvRelayout ? ev[i - 1].arg : -1;
    return -1;
  }
  // the real re-layout that ends the pass, -1: none
  constexpr int last() const { return ev[n_ev - 1].type == kEvRelayout ? ev[n_ev - 1].arg : -1; }
  // does e name the re-layout from -> to: a layout change is re-layout e, no
  // change is none
  constexpr bool names(int e, int from, int to) const {
    if (from == to) return e < 0;
    return e >= 0 && e < n_rl && e < kT12Masks && rl[e].from == from && rl[e].to == to;
  }
};

// pre / post: whether the pass has the kick layer, as the caller means it
constexpr PassProgram pass_program(int nibs, bool pre, bool post) {
  PassProgram p{};
  const int IO = io_layout(nibs), O = 3 - IO;
  const bool n0 = nibs & 1, nIO = (nibs >> IO) & 1, nO = (nibs >> O) & 1;
  p.IO = IO;
  p.O = O;
  p.k0 = n0 ? 0 : IO;
  p.d_lay = pre ? (nO ? O : p.k0) : IO;
  p.pO = nO ? O : p.d_lay;
  p.p0 = n0 ? 0 : p.pO;
  p.pIO = nIO ? IO : p.p0;
  int lay = IO;
  auto kick = [&](int half, int nib) {
    if (lay != nib) {
      if (p.n_rl < kT12Masks) p.rl[p.n_rl] = PassRelayout{lay, nib};
      p.ev[p.n_ev++] = PassEvent{kEvRelayout, p.n_rl++};
      lay = nib;
    }
    if (half >= 0) p.ev[p.n_ev++] = PassEvent{kEvKick, 4 * half + nib};
  };
  if (pre) {
    if (nIO) kick(0, IO);
    if (n0) kick(0, 0);
    if (nO) kick(0, O);
  }
  p.ev[p.n_ev++] = PassEvent{kEvDiag, 0};
  if (post) {
    if (nO) kick(1, O);
    if (n0) kick(1, 0);
    if (nIO) kick(1, IO);
  }
  kick(-1, IO);  // back to the store's layout
  return p;
}

// no plan has more real re-layouts than the total record has mask words
constexpr bool pass_programs_fit() {
  for (int nibs = 1; nibs < 8; ++nibs)
    for (int s = 0; s < 4; ++s)
      if (pass_program(nibs, s & 1, s & 2).n_rl > kT12Masks) return false;
  return true;
}
static_assert(pass_programs_fit(), "a pass with more than kT12Masks real re-layouts");

// ---- the frame -----------------------------------------------------------------
// var: the standard record's variant (SiteMat::var: 2 = form B, 1 = sigma < 0)
DTC_PF_HD inline int frame_form_a(int var) { return (var >> 1) ^ 1; }
// the Z a kick leaves behind
DTC_PF_HD inline int frame_zbit(bool rx, int var) {
  return rx ? (var & 1) : ((var & 1) ^ frame_form_a(var));
}

struct PauliFrame {
  int x = 0, z = 0, ph = 0;  // masks over tile bits; the power of i (not reduced)

  // the kick (var, coef) on tile bit `bit`: returns the signed form-B
  // coefficient to run, the frame takes the kick's Paulis
  DTC_PF_HD double kick(bool rx, int var, double coef, int bit) {
    const int fa = frame_form_a(var), n2 = frame_zbit(rx, var);
    const double g = fa ? -coef : coef;
    const int flip = ((rx ? z : (x ^ z)) >> bit) & 1;
    ph += (rx ? 3 * fa : 2 * fa) + 2 * flip;
    x ^= fa << bit;
    ph += 2 * (n2 & (x >> bit) & 1);
    z ^= n2 << bit;
    return flip ? -g : g;
  }
  // the computed tile comes out X^mask-permuted (a re-layout's write / read slots)
  DTC_PF_HD void flush_x(int mask) {
    ph += 2 * (__builtin_popcount(z & mask) & 1);
    x ^= mask;
  }
};

// ---- the frame of a 12-bit pass ------------------------------------------------
// X bits are flushed by the re-layouts (index y is written at slot(y ^ mw), read
// from slot(y ^ mr): the tile comes out X^(mw ^ mr)-permuted), Z bits at the
// diagonal point (a sign per amplitude: folded into the diagonal's tables; for
// a pass without one, the global factor's multiply; for a dual pass's echo
// branch, copied before the diagonal, its own sign flush), so that the frame is
// the identity at the diagonal and at the store.  A kicked nibble's X goes to
// the first re-layout after it within its half, on the read side (the sites are
// register bits of that re-layout's source layout, thread bits of its target:
// mr), else -- the half's last nibble -- to the last one before it, on the write
// side (register bits of the target, thread bits of the source: mw; pre-flushed:
// RX commutes it, RY flips g).  Either way the mask stays off the side's
// register offsets.  The Z of the post-kicks is pulled back through them to the
// diagonal point (npost: their bits depend on the variants only).  (A pass
// without any re-layout -- the IO nibble alone -- keeps its X: the kernel runs
// no such pass in frame form.)
struct Frame12 {
  double coef[2 * kPassBits];     // the signed G coefficient of (half, tile bit)
  int mw[kT12Masks], mr[kT12Masks];  // re-layout e's write-side / read-side X masks
  int md;                         // the Z mask of the diagonal point
  int ph;                         // the frame's extra power of i, 0..3
  PauliFrame end;                 // the frame left at the store
};

// var, coef: the standard records' variant and coefficient of (half, tile bit),
// at [half * kPassBits + bit]
DTC_PF_HD inline void frame12_walk(bool rx, int nibs, bool pre, bool post, const int* var,
                                   const double* coef, Frame12& o) {
  const PassProgram P = pass_program(nibs, pre, post);
  for (int i = 0; i < 2 * kPassBits; ++i) o.coef[i] = 0.0;
  for (int e = 0; e < kT12Masks; ++e) o.mw[e] = o.mr[e] = 0;
  for (int i = 0; i < P.n_ev; ++i) {
    if (P.ev[i].type != kEvKick) continue;
    const int nib = P.ev[i].arg & 3, i0 = (P.ev[i].arg >> 2) * kPassBits;
    int m = 0;
    for (int k = 4 * nib; k < 4 * nib + 4; ++k) m |= frame_form_a(var[i0 + k]) << k;
    int after = -1, before = -1;
    for (int f = i + 1; f < P.n_ev && P.ev[f].type != kEvDiag && after < 0; ++f)
      if (P.ev[f].type == kEvRelayout) after = P.ev[f].arg;
    for (int f = 0; f < i; ++f)
      if (P.ev[f].type == kEvRelayout) before = P.ev[f].arg;
    if (after >= 0) o.mr[after] |= m;
    else if (before >= 0) o.mw[before] |= m;
  }
  int npost = 0;
  if (post)
    for (int k = 0; k < kPassBits; ++k)
      if ((nibs >> (k >> 2)) & 1) npost |= frame_zbit(rx, var[kPassBits + k]) << k;
  PauliFrame f;
  o.md = 0;
  for (int i = 0; i < P.n_ev; ++i) {
    const PassEvent ev = P.ev[i];
    if (ev.type == kEvRelayout) {
      f.flush_x(o.mw[ev.arg] ^ o.mr[ev.arg]);
    } else if (ev.type == kEvDiag) {
      o.md = f.z ^ npost;
      f.z = npost;
    } else {
      const int i0 = (ev.arg >> 2) * kPassBits + 4 * (ev.arg & 3);
      for (int q = 0; q < 4; ++q)
        o.coef[i0 + q] = f.kick(rx, var[i0 + q], coef[i0 + q], 4 * (ev.arg & 3) + q);
    }
  }
  o.ph = f.ph & 3;
  o.end = f;
}

}  // namespace dtc
#undef DTC_PF_HD
