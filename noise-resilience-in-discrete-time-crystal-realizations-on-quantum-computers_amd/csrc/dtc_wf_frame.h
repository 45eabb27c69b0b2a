// dtc_wf_frame.h -- the Pauli frame of one wavefront launch (dtc_wavefront.hip),
// host and device: the prep kernel runs it per state (dtc_kernels.hip), and
// tools/wavefront_frame_check.cpp runs the same code on the CPU against the
// direct 2x2 products.
//
// The pass runs one butterfly for every kick, the form-B one G(f) (RX: f I +
// i X; RY: f I + i Y), as frame12_records / frame13_records do for the plain
// passes: form A is A(beta) = -i X G(-beta) (RX) or X Z G(-beta) (RY),
// sigma = -1 a Z after the kick.  The true tile is i^ph X^x Z^z (the computed
// tile); a kick Z^n X^a G(g) on tile bit k runs as G(+-g) (G past the frame:
// RX flips g with Z_k, RY with X_k xor Z_k) and the frame takes Z^n X^a.
// Unlike the plain passes nothing is flushed on the way: X stays in the frame
// to the store, and a partial diagonal under the frame X^x is the same table
// read at index y ^ x -- the kernel stages its per-workgroup tables with that
// XOR.  Z commutes with the diagonals; it leaves as a sign on the last
// diagonal's staged entries, together with the Z of the kicks that follow that
// diagonal pulled back through them (frame12_walk's npost; their bits depend
// on the variants only), so the frame is X^x alone at the store, which writes
// tile index y to y ^ x.  (A launch without any diagonal signs the tile where
// it applies the global factor.)
//
// Steps as the kernel runs them: a diagonal before step st where dmask has bit
// st (bit n_steps: the trailing one), then the butterflies of every nibble
// that mask[st] touches, on all of the nibble's site bits (`act`: a site that
// mask[st] leaves out carries the identity record, variant 0 with coefficient
// 0, which is G(0) with an X for the frame like any form A).  The order of the
// nibbles within a step does not matter here: a step kicks a site once and the
// frame is a product over sites.
#pragma once
#include <stdint.h>

#include "dtc_pass_frame.h"  // PauliFrame: the per-kick frame step

// (no HIP header: the CPU check compiles this file with a plain host
// compiler; dtc_kernels.hip asserts that the two constants are WfArgs')
#ifdef __HIPCC__
#define DTC_WF_HD __host__ __device__
#else
#define DTC_WF_HD
#endif

namespace dtc {

static constexpr int kWfFrameSteps = 4;   // kWfSteps
static constexpr int kWfFrameBits = 12;   // kTileBits

struct WfFrame {
  double coef[kWfFrameSteps][kWfFrameBits];  // the signed G coefficient of (step, tile bit)
  uint64_t xdiag;  // bits 12 st .. 12 st + 11: the frame's X at the diagonal of step st
  int zlast;       // the Z mask folded into the last diagonal applied (none: at the end)
  int xend;        // the frame's X at the store
  int ph;          // the frame's extra power of i
};

// the tile bits whose butterflies run in a step that kicks `mask`
DTC_WF_HD inline int wf_step_bits(uint32_t mask, int act) {
  int m = 0;
  for (int n = 0; n < 3; ++n)
    if (mask & (0xFu << (4 * n))) m |= 0xF << (4 * n);
  return m & act;
}

// var, coef: the standard records' variant (SiteMat::var) and coefficient of
// (step, tile bit)
DTC_WF_HD inline void wf_frame_walk(bool rx, int n_steps, const uint32_t* mask, int dmask,
                                    int act, const int (*var)[kWfFrameBits],
                                    const double (*coef)[kWfFrameBits], WfFrame& o) {
  auto zbit = [&](int st, int k) { return frame_zbit(rx, var[st][k]); };
  // where Z leaves: the last diagonal applied, or the end of a launch without
  // any (the kernel then signs the tile with its global factor)
  int last = n_steps;
  for (int st = 0; st < n_steps; ++st)
    if ((dmask >> st) & 1) last = st;
  if ((dmask >> n_steps) & 1) last = n_steps;
  int npost = 0;
  for (int st = last; st < n_steps; ++st) {
    const int bits = wf_step_bits(mask[st], act);
    for (int k = 0; k < kWfFrameBits; ++k)
      if ((bits >> k) & 1) npost ^= zbit(st, k) << k;
  }
  PauliFrame f;
  o.xdiag = 0;
  o.zlast = 0;
  for (int st = 0; st <= n_steps; ++st) {
    if ((dmask >> st) & 1) o.xdiag |= (uint64_t)f.x << (kWfFrameBits * st);
    if (st == last) {
      o.zlast = f.z ^ npost;
      f.z = npost;
    }
    for (int k = 0; k < kWfFrameBits; ++k) {
      if (st < kWfFrameSteps) o.coef[st][k] = 0.0;
      if (st == n_steps || !((wf_step_bits(mask[st], act) >> k) & 1)) continue;
      o.coef[st][k] = f.kick(rx, var[st][k], coef[st][k], k);
    }
  }
  for (int st = n_steps + 1; st < kWfFrameSteps; ++st)
    for (int k = 0; k < kWfFrameBits; ++k) o.coef[st][k] = 0.0;
  o.xend = f.x;
  o.ph = f.ph & 3;
}

// ---- tile 2's partial diagonal in layout 1 -----------------------------------
// Tile 2 (tile bits 0..2 = columns, bit k >= 3 = site k + 8) snakes between
// layouts 2 and 1 only (dtc_wavefront.hip), so the diagonals of its odd steps
// are applied in layout 1: registers = tile bits 4..7, thread = bits 0..3 and
// 8..11.  The step's factors regroup into
//   the register table, 64 entries over tile bits 3..8: everything that touches
//     a register bit -- fields 4..7, bonds (3,4) .. (7,8) -- read as thread
//     base (bits 3, 8) + register offset (r << 1);
//   the thread table, 32 entries over tile bits 3, 8..11: the rest -- field 3
//     with the outside bond, fields 8..11, bonds (8,9) .. (10,11) -- one
//     thread-constant entry.
// Each factor is in exactly one table.  They sit at [0, 64) and [64, 96) of the
// step's kWfTab-entry slot.  Under the frame both are staged as the 0..6 / 6..11
// pair is: entry i at i ^ (the frame's X gathered onto the table's index bits),
// the last diagonal's Z as the parity of the staged index under the gathered Z
// mask; bits 3 and 8 index both tables and count in the register table only.
static constexpr int kWfL1Reg = 64;  // register-table entries
static constexpr int kWfL1Thr = 32;  // thread-table entries

DTC_WF_HD inline bool wf_l1_reg_bit(int k) { return k >= 4 && k <= 7; }
// position of tile bit k in a table's index, -1 where the table has no such bit
DTC_WF_HD inline int wf_l1_reg_pos(int k) { return (k >= 3 && k <= 8) ? k - 3 : -1; }
DTC_WF_HD inline int wf_l1_thr_pos(int k) { return k == 3 ? 0 : ((k >= 8 && k <= 11) ? k - 7 : -1); }
// a tile index (or an X mask) gathered onto the tables' index bits
DTC_WF_HD inline int wf_l1_reg_index(int y) { return (y >> 3) & 63; }
DTC_WF_HD inline int wf_l1_thr_index(int y) { return ((y >> 3) & 1) | (((y >> 8) & 15) << 1); }
// a Z mask gathered likewise, bits 3 and 8 left to the register table
DTC_WF_HD inline int wf_l1_reg_zmask(int z) { return (z >> 3) & 63; }
DTC_WF_HD inline int wf_l1_thr_zmask(int z) { return ((z >> 9) & 7) << 2; }
// the table of a factor on tile bit k (a field, or a bond to a bit outside the
// tile: k2 < 0) or on bits k, k2 (a bond inside the tile): true = register
DTC_WF_HD inline bool wf_l1_in_reg(int k, int k2) {
  return wf_l1_reg_bit(k) || (k2 >= 0 && wf_l1_reg_bit(k2));
}

// ---- the thread's own table entry, fetched from the global table --------------
// A diagonal reads one of its slot's two tables per register and the other
// once per thread (dtc_wavefront.hip, wf_diag).  Only the per-register table is
// staged in LDS; the thread takes its constant straight from the slot's global
// table (kWfTabA + kWfTabB entries as wf_table_set fills them), applying the
// staging's X permutation and Z sign itself: with i the thread's index into
// the staged table, the entry is global[i ^ x] (x = the step's frame X gathered
// onto the table's index bits), negated in the last diagonal by the parity of i
// under the gathered Z mask -- the value a staged table holds at i.
// lay: the layout the diagonal runs in (2: even slots; 0: tile 1's odd slots;
// 1: tile 2's odd slots); y: the thread's tile index base, ybase<lay>(t).
static constexpr int kWfFetchTabA = 128;  // kWfTabA
DTC_WF_HD inline int wf_thr_staged(int lay, int y) {
  return lay == 2 ? (y & (kWfFetchTabA - 1)) : (lay == 0 ? ((y >> 6) & 63) : wf_l1_thr_index(y));
}
// offset of the thread's entry in the slot's global table under the frame X fx
DTC_WF_HD inline int wf_thr_fetch(int lay, int y, int fx) {
  const int i = wf_thr_staged(lay, y);
  if (lay == 2) return i ^ (fx & (kWfFetchTabA - 1));
  if (lay == 0) return kWfFetchTabA + (i ^ ((fx >> 6) & 63));
  return kWfL1Reg + (i ^ wf_l1_thr_index(fx));
}
// the last diagonal's sign of that entry under the frame Z fz (tile bit 6, and
// in layout 1 bits 3 and 8, count in the other table)
DTC_WF_HD inline bool wf_thr_neg(int lay, int y, int fz) {
  const int zm = lay == 2 ? (fz & 63) : (lay == 0 ? ((fz >> 6) & 63) : wf_l1_thr_zmask(fz));
  int p = wf_thr_staged(lay, y) & zm;
  p ^= p >> 4;
  p ^= p >> 2;
  p ^= p >> 1;
  return p & 1;
}
// The per-register table of a slot, the one LDS keeps: its offset and size in
// the slot's global table, and the X / Z masks gathered onto its index.
DTC_WF_HD inline int wf_reg_base(int lay) { return lay == 2 ? kWfFetchTabA : 0; }
DTC_WF_HD inline int wf_reg_size(int lay) { return lay == 0 ? kWfFetchTabA : 64; }
DTC_WF_HD inline int wf_reg_xmask(int lay, int fx) {
  return lay == 2 ? ((fx >> 6) & 63) : (lay == 0 ? (fx & (kWfFetchTabA - 1)) : wf_l1_reg_index(fx));
}
DTC_WF_HD inline int wf_reg_zmask(int lay, int fz) {
  return lay == 2 ? ((fz >> 6) & 63) : (lay == 0 ? (fz & 63) : wf_l1_reg_zmask(fz));
}

// ---- layout 0's register table in LDS -----------------------------------------
// The 128-entry table over tile bits 0..6 is read per register at row (tile
// bits 4..6, the thread's) and column (bits 0..3, the register): entry j sits at
// wf_pad0(j), rows of 17 entries, kWfTabA0 entries in all.  ds_read_b128 serves
// 16 lanes per LDS cycle, 64 banks of 4 B: rows of 16 entries (256 B) put a
// group's eight rows on the same four banks; rows of 17 put them four banks
// apart (tools/wavefront_t1_swap_check.cpp checks the lane groups).
DTC_WF_HD constexpr int wf_pad0(int j) { return j + (j >> 4); }
static constexpr int kWfTabA0 = (wf_pad0(kWfFetchTabA - 1) + 1 + 3) & ~3;  // 136

// ---- tile 1's swap form: four layouts, one LDS re-layout per kick step --------
// (dtc_wavefront.hip, DTC_WF_T1_SWAP; tools/wavefront_t1_swap_check.cpp runs
// these maps on the CPU.)  A thread is lane bits l0..5 = t & 63 and wave bits
// w0,1 = t >> 6; y0..11 are the tile index bits, r0..3 the register bits.
//   L2  (load / store): r = y8..11,             l0..5 = y0..5,        w = y6,7
//   L2s = L2 after the row swaps l4 <-> r0, l5 <-> r1:
//                       r = (y4, y5, y10, y11), l0..3 = y0..3, l4,5 = (y8, y9)
//   Q                 : r = y0..3,  l0..3 = (y4, y5, y8, y9), l4,5 = (y6, y7),
//                                                              w = (y10, y11)
//   Qs  = Q after the same two swaps:
//                       r = (y6, y7, y2, y3),                  l4,5 = (y0, y1)
// Sites in registers: 8..11, then 4, 5 in the L2 pair; 0..3, then 6, 7 in the
// Q pair.  The LDS re-layouts run between the swapped forms (L2s <-> Qs) and,
// behind a pass with an odd step count, Q -> L2.
enum { kWfLayL2 = 0, kWfLayL2s = 1, kWfLayQ = 2, kWfLayQs = 3 };

// tile index of thread t's register 0, and register r's offset on top of it
DTC_WF_HD constexpr int wf_t1_ybase(int lay, int t) {
  const int l03 = t & 15, l45 = (t >> 4) & 3, w = t >> 6;
  if (lay == kWfLayL2) return t;
  if (lay == kWfLayL2s) return l03 | (l45 << 8) | (w << 6);
  const int q = ((l03 & 3) << 4) | ((l03 >> 2) << 8) | (w << 10);
  return lay == kWfLayQ ? (q | (l45 << 6)) : (q | l45);
}
DTC_WF_HD constexpr int wf_t1_roff(int lay, int r) {
  if (lay == kWfLayL2) return r << 8;
  if (lay == kWfLayL2s) return ((r & 3) << 4) | ((r >> 2) << 10);
  if (lay == kWfLayQ) return r;
  return ((r & 3) << 6) | ((r >> 2) << 2);
}
// The slot of tile index y in the half-tile buffer (8-B slots), linear over
// XOR as slot_add is: low slot bits (y0^y4, y1^y5, y2^y8, y3^y9, y4^y8), the
// rest y5..y11.  A 16-lane group of a store (l0..3) must differ in slot bits
// 0..3 and a 32-lane group of a load (l0..4) in bits 0..4 to be free of bank
// conflicts (8-B slots: banks (2 slot) mod 32 and mod 64); this map does both
// for the lanes of L2 (y0..4), L2s (y0..3, y8) and Q / Qs (y4, y5, y8, y9 and
// y6 / y0), which slot_add does not (y9 reaches none of its low bits).
DTC_WF_HD constexpr int wf_t1_slot(int y) {
  return y ^ ((y >> 4) & 3) ^ (((y >> 8) & 3) << 2) ^ (((y >> 8) & 1) << 4);
}

}  // namespace dtc
#undef DTC_WF_HD
