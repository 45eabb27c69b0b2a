// dtc_wavefront.hip -- the stored wavefront pass: up to kWfSteps masked kick
// layers with partial diagonals before them over one 12-bit tile, one HBM read
// and write of the state for all of them (planner: dtc_wavefront.h; DESIGN.md
// section 4).  Two tiles: T1 = index bits 0..11 (sites 0..11), T2 = index bits
// 0..2 as 128-B columns + sites 11..19; the shared site 11 lets each pass lift
// its own sites by several layers.
//
// Kicks: the factored RX / RY butterflies of the plain passes in Pauli-frame
// form (dtc_wf_frame.h: one form-B butterfly per kick, no variant branch; the
// frame's X rides to the store, its Z to the last diagonal), from two
// consecutive standard record blocks per state (steps 0, 1 = the first
// block's pre / post layer, steps 2, 3 the second's; skipped tile bits carry
// identity records).  Diagonals: per (instance, step) a 128-entry
// table over tile bits 0..6 (their fields, the bonds among them) and a 64-entry
// table over bits 6..11, for the workgroup's value of the one index bit
// outside the tile that a bond reaches (a sign on the in-tile site's angle);
// the table a diagonal reads per register is staged in LDS, the thread's one
// entry of the other comes straight from the global table.
// Program: the tile snakes through the register layouts, 2 -> 1 -> 0 in even
// steps and 0 -> 1 -> 2 in odd ones, so every step costs two LDS re-layouts and
// the diagonals are applied in layouts 2 and 0 only.  T2's nibble 0 holds the
// one site 11, and tile bit 3 is lane bit 3 in layouts 1 and 2: T2 snakes
// 2 -> 1 and 1 -> 2 only, one re-layout per step,
// kicks site 11 across lanes (wf_kick_lane3) and applies its odd steps'
// diagonals in layout 1 from a register / thread table pair (dtc_wf_frame.h;
// profiles/r9_wavefront_chain_ab20.txt).  The re-layouts go through
// a half-tile buffer (exchange_split), so three workgroups share a CU: 8.9 ms
// per four-layer pass against 10.4 ms with the full tile at two per CU
// (profiles/r7_wavefront_ab20.txt); with the register tables alone beside the
// buffer and 115 VGPRs tile 1 runs at four per CU (DTC_WF_WG4 below).
#include <hip/hip_runtime.h>

#include "dtc_device.h"
#include "dtc_kernels.h"
#include "dtc_wf_frame.h"

// Three or four workgroups per CU (half-tile re-layouts) or two (full-tile)
#ifndef DTC_WF_SPLIT
#define DTC_WF_SPLIT 1
#endif
// The 1 <-> 0 re-layouts of tile 1 wave-local, without workgroup barriers
// (dtc_device.h exchange, WAVE): development A/B, off in the product -- 12 of a
// pass's 24 barriers gone bought 0.10 ms per launch and C2 +0.5 %, under the
// adoption bar (profiles/r9_wavefront_chain_ab20.txt)
#ifndef DTC_WF_WAVE_XCH
#define DTC_WF_WAVE_XCH 0
#endif
// Four workgroups per CU for the half-tile form, bit 0: tile 1, bit 1: the
// column tile.  The kernels fit either way (at most 128 VGPRs, under 40 KiB of
// LDS); a tile whose bit is off pads its LDS to stay at three per CU.  The
// product runs tile 1 at four (8.34 -> 8.01 ms per launch) and the column tile
// at three (at four it ran 7.41 -> 7.52 ms): C2 +1.8 % against +1.7 % with both
// at four and +0.0 % with neither (profiles/r10_wavefront_wg4_ab20.txt)
#ifndef DTC_WF_WG4
#define DTC_WF_WG4 1
#endif
// Tile 1's program: 0, the three-layout snake 2 -> 1 -> 0 (two LDS re-layouts
// per kick step); 1, the swap form -- sites 4, 5 and 6, 7 come into registers by
// row swaps (swap_reg_lane, no LDS), so one re-layout per kick step is left
// (the layouts and the slot map: dtc_wf_frame.h; the program: dtc_wf_pass).
// Development A/B, off in the product: the swap form is correct (every
// wavefront test passes with it, echo within 1.5e-15 of the snake's) and fits
// four workgroups per CU (118 VGPRs, no more LDS, no scratch), but the 128 row
// swaps per step cost what the re-layout they replace did: C2 -0.2 % and
// -0.7 % in two pairs (profiles/r12_wavefront_t1_swap_ab20.txt)
#ifndef DTC_WF_T1_SWAP
#define DTC_WF_T1_SWAP 0
#endif

namespace dtc {

// v[r] *= (fac * e) * TR[..] in layout LAY: e is the thread's own entry of the
// table that is constant per thread (fetched from the global table, wf_fetch
// below), TR the slot's per-register table in LDS.  Layout 2: registers = tile
// bits 8..11, TR the 6..11 table; 0: registers = bits 0..3, TR the 0..6 table;
// 1, the column tile's odd steps: registers = bits 4..7, TR the register table
// of dtc_wf_frame.h.  The table is read four entries at a time with their
// products in between (a scheduling barrier per group), so the sixteen entries
// are never all live on top of the tile: the pass fits 128 VGPRs.
// T1Q (layout 0 only): the swap form's layout Q, registers = bits 0..3 as in
// layout 0 and the same two tables, the thread's tile bits 4..6 from its own map.
//
// Layout 0's table sits in LDS in rows of 17 (wf_pad0, dtc_wf_frame.h): a lane
// reads row (tile bits 4..6) at the register's column, and with rows of 16
// entries = 256 B the eight rows of a ds_read_b128 lane group fell on the same
// four banks, an 8-way conflict on every read (SQ_LDS_BANK_CONFLICT: 655 cycles
// per wave of 2 196 LDS cycles; profiles/r12_wavefront_t1_swap_ab20.txt).
template <int LAY, bool T1Q = false>
__device__ __forceinline__ void wf_diag(double2 (&v)[kRegs], const double2* slot, int t,
                                        double2 fac, double2 e) {
  static_assert(LAY >= 0 && LAY <= 2 && (!T1Q || LAY == 0), "tile layout");
  const double2 c = cmul(fac, e);
  const double2* tr = slot + (LAY == 1   ? wf_l1_reg_index(ybase<1>(t))
                              : LAY == 2 ? ((t >> 6) & 3)
                              : T1Q      ? wf_pad0(wf_t1_ybase(kWfLayQ, t) & 0x70)
                                         : wf_pad0((t & 7) << 4));
  constexpr int kStep = LAY == 1 ? 2 : (LAY == 2 ? 4 : 1);
#pragma unroll
  for (int g = 0; g < kRegs; g += 4) {
#pragma unroll
    for (int r = g; r < g + 4; ++r) v[r] = cmul(v[r], cmul(c, tr[r * kStep]));
    __builtin_amdgcn_sched_barrier(0);
  }
}

// Frame-form kick (form B, coefficient f) of tile bit 3 where it is lane bit 3
// (layouts 1 and 2): the partner amplitude is lane l ^ 8's, one row_ror:8 DPP
// move per dword, and each lane computes its own row of the butterfly.  RX:
// S = [[f, i], [i, f]] is symmetric, both lanes run bfly_rx_f<2>'s nu; RY:
// R = [[f, 1], [-1, f]], the partner enters with the sign of lane bit 3.  The
// fma shapes are bfly_*_f<2>'s, so the rounding is the register form's.
template <int KIND>
__device__ __forceinline__ void wf_kick_lane3(double2 (&v)[kRegs], double f) {
  const long long sm = (KIND == kKindRY && (__lane_id() & 8)) ? (long long)(1ull << 63) : 0ll;
#pragma unroll
  for (int r = 0; r < kRegs; ++r) {
    const double px = xor_lane<8>(v[r].x), py = xor_lane<8>(v[r].y);
    if (KIND == kKindRX) {
      v[r] = make_double2(fma(f, v[r].x, -py), fma(f, v[r].y, px));
    } else {
      v[r] = make_double2(fma(f, v[r].x, __longlong_as_double(__double_as_longlong(px) ^ sm)),
                          fma(f, v[r].y, __longlong_as_double(__double_as_longlong(py) ^ sm)));
    }
  }
}

// The swap form's LDS re-layouts (tile 1, DTC_WF_T1_SWAP): L2s -> Qs, Qs -> L2s
// and Q -> L2 through the half-tile buffer in exchange_split's discipline --
// real parts, then imaginary parts, a slot the thread's base XOR a compile-time
// register offset -- with the slot map of dtc_wf_frame.h, under which every
// store and load of the three is free of bank conflicts
// (tools/wavefront_t1_swap_check.cpp).  No barrier before the writes of the
// first two: the tile is in the same swapped layout whenever it leaves for LDS
// or comes back, so a thread writes the slots it read itself last.  Q -> L2
// writes from Q what came back in Qs: the caller puts a barrier in front of it.
template <int FROM, int TO>
__device__ __forceinline__ void exchange_t1(double2 (&v)[kRegs], double* s_half, int t) {
  int bf = wf_t1_slot(wf_t1_ybase(FROM, t)), bt = wf_t1_slot(wf_t1_ybase(TO, t));
  asm volatile("" : "+v"(bf), "+v"(bt));  // formed afresh per exchange (exchange_split)
#pragma unroll
  for (int r = 0; r < kRegs; ++r) s_half[bf ^ wf_t1_slot(wf_t1_roff(FROM, r))] = v[r].x;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kRegs; ++r) v[r].x = s_half[bt ^ wf_t1_slot(wf_t1_roff(TO, r))];
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kRegs; ++r) s_half[bf ^ wf_t1_slot(wf_t1_roff(FROM, r))] = v[r].y;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kRegs; ++r) v[r].y = s_half[bt ^ wf_t1_slot(wf_t1_roff(TO, r))];
}

// register bits 0, 1 <-> lane bits 4, 5: L2 <-> L2s and Q <-> Qs
__device__ __forceinline__ void wf_t1_swap(double2 (&v)[kRegs]) {
  swap_reg_lane<0, 16>(v);
  swap_reg_lane<1, 32>(v);
}

// LDS keeps the per-register table of every slot only (dtc_wf_frame.h): 64
// entries for the even slots and the column tile's odd ones, kWfTabA in rows of
// 17 (kWfTabA0, wf_diag) for tile 1's odd ones.  Slot st's offset, and the
// whole array, in entries:
__host__ __device__ constexpr int wf_slot_ofs(bool two_lay, int st) {
  return two_lay ? st * kWfTabB : (st >> 1) * (kWfTabB + kWfTabA0) + (st & 1) * kWfTabB;
}
__host__ __device__ constexpr int wf_tab_lds(bool two_lay) { return wf_slot_ofs(two_lay, kWfSteps + 1); }
static_assert(kWfTabB == 64 && kWfL1Reg == 64 && kWfTabA == kWfFetchTabA && (kWfSteps & 1) == 0,
              "the register tables of dtc_wf_frame.h");

// Whether a tile's half-tile form runs at four workgroups per CU: its bit of
// DTC_WF_WG4, and only where the re-layout buffer and the register tables fit
// a quarter of the CU's 160 KiB (a development build with the larger additive
// slots, DTC_ADD_SLOTS, does not, and stays at three)
__host__ __device__ constexpr bool wf_wg4(int qm0) {
  return ((DTC_WF_WG4 >> (qm0 == 8)) & 1) &&
         sizeof(double) * kHalfSlots + sizeof(double2) * wf_tab_lds(kWfT2Lay1 && qm0 == 8) <=
             160 * 1024 / 4;
}

template <int KIND, int QM0, bool SPLIT>
__global__ __launch_bounds__(kThreads, SPLIT ? (wf_wg4(QM0) ? 4 : 3) : 2) void dtc_wf_pass(WfArgs A) {
  constexpr bool kWg4 = SPLIT && wf_wg4(QM0);
  // The column tile (QM0 = 8: nibble 0 holds the one site 11, tile bit 3) never
  // visits layout 0: bit 3 is lane bit 3 in layouts 1 and 2, so its kick runs
  // across lanes (wf_kick_lane3) and the odd steps' diagonals are applied in
  // layout 1 -- two re-layouts per step pair instead of four, all cross-wave.
  constexpr bool kTwoLay = kWfT2Lay1 && QM0 == 8;
  // Tile 1 in the swap form (DTC_WF_T1_SWAP): layouts L2, L2s, Q, Qs of
  // dtc_wf_frame.h, the odd slots' diagonals in Q with layout 0's tables
  constexpr bool kT1Swap = DTC_WF_T1_SWAP != 0 && SPLIT && QM0 == 15;
  // SPLIT: the re-layouts through a half-tile buffer (real parts, then
  // imaginary parts); with the register tables alone beside it, 40 192 B
  // (tile 1, its layout-0 tables in rows of 17) and 37 888 B (the column
  // tile): four workgroups fit a CU's LDS
  __shared__ double2 s_tile[SPLIT ? 1 : kTile];
  __shared__ double s_half[SPLIT ? kHalfSlots : 1];
  // A tile that is to stay at three per CU pads s_tab to the full tables'
  // size, 48 128 B in all.  The padding is dead LDS, there only as an occupancy
  // limiter: the launch bounds promise a least occupancy, they are no cap, and
  // the kernel's own 37 888 B and 114 VGPRs would fit a fourth workgroup.
  // wf_slot_ofs stays the compact one either way.
  __shared__ double2 s_tab[kWg4 || !SPLIT ? wf_tab_lds(kTwoLay) : (kWfSteps + 1) * kWfTab];
  static_assert(!kWg4 || sizeof(s_half) + sizeof(s_tab) <= 160 * 1024 / 4, "four workgroups per CU");
  static_assert(wf_tab_lds(kTwoLay) <= (kWfSteps + 1) * kWfTab, "the padded form holds the tables");

  const int t = threadIdx.x;
  const int og = A.octet_bits;
  const int64_t b = og ? (((int64_t)blockIdx.y << 3) | (blockIdx.x & 7)) : (int64_t)blockIdx.y;
  const int64_t tile = og ? (int64_t)(blockIdx.x >> 3) : (int64_t)blockIdx.x;
  if (b >= A.batch) return;  // the padding states of a last partial octet
  const int inst = (int)((A.batch_start + b) / A.n_traj);
  const int n = A.n_steps;
  // the layout of the odd slots' diagonals
  constexpr int kOddLay = kTwoLay ? 1 : 0;

  TileMap M;
  M.c = A.c;
  M.s = A.s;
  M.cmask = (1 << A.c) - 1;
  const int mid = A.s - A.c;
  M.tbase = ((tile & (((int64_t)1 << mid) - 1)) << A.c) | ((tile >> mid) << (A.s + kTileBits - A.c));

  // the steps' register tables for this workgroup's outside bit, before the
  // tile's loads
  const int var = A.out_bit >= 0 ? (int)((M.tbase >> A.out_bit) & 1) : 0;
  const double2* tg = A.tab + ((int64_t)inst * (kWfSteps + 1) * 2 + var) * kWfTab;
  double2 stage[kWfSteps + 1];
#pragma unroll
  for (int st = 0; st <= kWfSteps; ++st) {
    const int lay = (st & 1) ? kOddLay : 2;
    stage[st] = make_double2(1.0, 0.0);
    if (t < wf_reg_size(lay) && ((A.dmask >> st) & 1))
      stage[st] = tg[st * 2 * kWfTab + wf_reg_base(lay) + t];
  }

  const int64_t sbase = state_base(b, A.state_len, og);
  const int64_t vofs = octet_spread(M.at(ybase<2>(t)), og);
  double2 v[kRegs];
  {
    const double2* src = A.src + sbase + vofs;
#pragma unroll
    for (int r = 0; r < kRegs; ++r) {
      const d2v w =
          __builtin_nontemporal_load((const d2v*)(src + octet_spread(M.rel(r << 8), og)));
      v[r] = make_double2(w.x, w.y);
    }
  }
  // The Pauli frame of the launch (dtc_wf_frame.h; masks in the second block's
  // total record): the tables of step st are read X-permuted by the frame's X
  // at that diagonal -- entry i ^ x at i, each table with its part of the mask
  // -- and the last diagonal's take the Z flush as a sign per entry (a parity
  // of the index read; tile bit 6 counts in the 6..11 table).  The register
  // tables are staged so, at the LDS write, and the thread's own entries are
  // fetched so (wf_fetch): the scalar loads of the masks wait behind the
  // tile's loads, not in front of them.
  const RecScalar R0(A.recs + b * kRecPerState);
  const RecScalar R1(A.recs + ((int64_t)A.batch + b) * kRecPerState);
  const long long fxd = R1.bits(8 * kRecTotal + kWfMaskXD);
  const int fzx = R1.i(kRecTotal, kWfMaskZX);
  const int last = 31 - __builtin_clz(A.dmask | 1);
  // The entry of step st's per-thread table that this thread multiplies by,
  // from the global table (1 where the step has no diagonal).  Fetched one
  // diagonal ahead, so one entry is live at a time and its latency hides
  // behind the kicks and re-layouts in between.
  auto wf_fetch = [&](auto lay, int st) {
    constexpr int LAY = decltype(lay)::value;
    // (layout 0 of the swap form is Q: the same tables, its own thread map)
    const int yb = (kT1Swap && LAY == 0) ? wf_t1_ybase(kWfLayQ, t) : ybase<LAY>(t);
    double2 e = make_double2(1.0, 0.0);
    if ((A.dmask >> st) & 1) {
      const int fx = (int)(fxd >> (kTileBits * st)) & (kTile - 1);
      e = tg[st * 2 * kWfTab + wf_thr_fetch(LAY, yb, fx)];
      if (st == last && wf_thr_neg(LAY, yb, fzx & (kTile - 1))) e = make_double2(-e.x, -e.y);
    }
    return e;
  };
  using L0 = std::integral_constant<int, 0>;
  using L1 = std::integral_constant<int, 1>;
  using L2 = std::integral_constant<int, 2>;
  using LOdd = std::integral_constant<int, kOddLay>;
  double2 cn = wf_fetch(L2{}, 0);
  if (t < kWfTabA) {
    const int fz = fzx & (kTile - 1);
#pragma unroll
    for (int st = 0; st <= kWfSteps; ++st) {
      const int lay = (st & 1) ? kOddLay : 2;
      if (t >= wf_reg_size(lay) || !((A.dmask >> st) & 1)) continue;
      const int fx = (int)(fxd >> (kTileBits * st)) & (kTile - 1);
      const int j = t ^ wf_reg_xmask(lay, fx);
      const bool neg = st == last && (__popc(j & wf_reg_zmask(lay, fz)) & 1);
      s_tab[wf_slot_ofs(kTwoLay, st) + (lay == 0 ? wf_pad0(j) : j)] =
          neg ? make_double2(-stage[st].x, -stage[st].y) : stage[st];
    }
  }
  __syncthreads();

  // the kicks' global factor (both record blocks', the frame's power of i in
  // the second), folded into the first diagonal applied
  double2 gf = cmul(make_double2(R0.d(kRecTotal, 0), R0.d(kRecTotal, 1)),
                    make_double2(R1.d(kRecTotal, 0), R1.d(kRecTotal, 1)));
  // the diagonal before step st with the entry fetched for it; then the fetch
  // for the next one, slot nx in layout nlay (the next step's or the trailing
  // one; past those dmask has no bit)
  auto diag = [&](auto lay, int st, auto nlay, int nx) {
    if ((A.dmask >> st) & 1) {
      constexpr int LAY = decltype(lay)::value;
      wf_diag<LAY, kT1Swap && LAY == 0>(v, s_tab + wf_slot_ofs(kTwoLay, st), t, gf, cn);
      gf = make_double2(1.0, 0.0);
    }
    if (nx <= kWfSteps) cn = wf_fetch(nlay, nx);
  };
  auto kick = [&](auto nib, int st) {
    constexpr int N = decltype(nib)::value;
    if (!(A.mask[st] & (0xFu << (4 * N)))) return;
    const RecScalar R(A.recs + ((int64_t)(st >> 1) * A.batch + b) * kRecPerState);
    apply_nibble<N, KIND, N == 0 ? QM0 : 15, /*FRAME=*/true>(v, R, (st & 1) * kTileBits);
  };
  // The swap form's kicks of nibble 1, two sites at a time where a row swap
  // has them in register bits 0, 1: sites 4, 5 in L2s (H = 0), 6, 7 in Qs
  // (H = 1).  The nibble runs whole or not at all, as kick() has it: the
  // frame counts a butterfly on each of its sites (dtc_wf_frame.h).
  auto kick_pair = [&](auto half, int st) {
    constexpr int H = decltype(half)::value;
    if (!(A.mask[st] & 0xF0u)) return;
    const RecScalar R(A.recs + ((int64_t)(st >> 1) * A.batch + b) * kRecPerState);
    const int k = (st & 1) * kTileBits + 4 + 2 * H;
    layer_f<KIND, 2, 0>(v, R.d(k, 3));
    layer_f<KIND, 2, 1>(v, R.d(k + 1, 3));
  };
  // no flush masks are passed to the re-layouts (the frame's X leaves at the
  // store), so the 1 <-> 0 pair stays inside each wave (DTC_WF_WAVE_XCH)
  constexpr bool kWaveXch = DTC_WF_WAVE_XCH != 0;

  // site 11 of the column tile, across lanes (skipped like kick() when the
  // step's mask leaves it out)
  auto kick3 = [&](int st) {
    if (!(A.mask[st] & 8u)) return;
    const RecScalar R(A.recs + ((int64_t)(st >> 1) * A.batch + b) * kRecPerState);
    wf_kick_lane3<KIND>(v, R.d((st & 1) * kTileBits + 3, 3));
  };

  // The trailing kick-less step runs as the loop's own diagonal of its parity
  // (one copy of each diagonal in the code, and the tile stays in the loop's
  // registers: a second copy behind the loop cost 112 B per lane of scratch at
  // 128 VGPRs); a pass with an odd step count then leaves the loop in the odd
  // slots' layout and goes back to the load / store layout behind it.
  // (a bottom-tested loop: rotating a top-tested one would clone the first
  // diagonal in front of it again)
  int st = 0;
  if constexpr (kT1Swap) {
    // One re-layout per kick step: even steps run L2 -> L2s | Qs -> Q, odd
    // ones back, the diagonals in the unswapped L2 and Q.  The swaps always
    // run, whatever the step's mask (the re-layouts exist in one form each).
    using H0 = std::integral_constant<int, 0>;
    using H1 = std::integral_constant<int, 1>;
#pragma unroll 1
    do {
      diag(L2{}, st, L0{}, st + 1);
      if (st < n) {
        kick(L2{}, st);
        wf_t1_swap(v);
        kick_pair(H0{}, st);
        exchange_t1<kWfLayL2s, kWfLayQs>(v, s_half, t);
        kick_pair(H1{}, st);
        wf_t1_swap(v);
        kick(L0{}, st);
        diag(L0{}, st + 1, L2{}, st + 2);
        if (st + 1 < n) {
          kick(L0{}, st + 1);
          wf_t1_swap(v);
          kick_pair(H1{}, st + 1);
          exchange_t1<kWfLayQs, kWfLayL2s>(v, s_half, t);
          kick_pair(H0{}, st + 1);
          wf_t1_swap(v);
          kick(L2{}, st + 1);
        }
      }
      st += 2;
    } while (st <= n);
    if (n & 1) {
      __syncthreads();  // the writes from Q are not the slots read in Qs
      exchange_t1<kWfLayQ, kWfLayL2>(v, s_half, t);
    }
  } else {
#pragma unroll 1
    do {
      diag(L2{}, st, LOdd{}, st + 1);
      if (st < n) {
        kick(L2{}, st);
        xch_tile<SPLIT, 2, 1>(v, s_tile, s_half, t);
        kick(L1{}, st);
        if constexpr (kTwoLay) {
          kick3(st);
        } else {
          xch_tile<SPLIT, 1, 0, kWaveXch>(v, s_tile, s_half, t);
          kick(L0{}, st);
        }
        diag(LOdd{}, st + 1, L2{}, st + 2);
        if (st + 1 < n) {
          if constexpr (kTwoLay) {
            kick3(st + 1);
            kick(L1{}, st + 1);
          } else {
            kick(L0{}, st + 1);
            xch_tile<SPLIT, 0, 1, kWaveXch>(v, s_tile, s_half, t);
            kick(L1{}, st + 1);
          }
          xch_tile<SPLIT, 1, 2>(v, s_tile, s_half, t);
          kick(L2{}, st + 1);
        }
      }
      st += 2;
    } while (st <= n);
    if (n & 1) xch_tile<SPLIT, kOddLay, 2>(v, s_tile, s_half, t);
  }
  // a launch without any diagonal: the global factor and the frame's Z here
  // (layout 2: the thread's bits 0..7, the registers' 8..11)
  if (!A.dmask) {
    const int fz = fzx & (kTile - 1);
    const double sg = (__popc(t & fz) & 1) ? -1.0 : 1.0;
#pragma unroll
    for (int r = 0; r < kRegs; ++r) {
      const double s = (__popc(r & (fz >> 8)) & 1) ? -sg : sg;
      v[r] = cmul(v[r], make_double2(s * gf.x, s * gf.y));
    }
  }
  // The frame's X leaves at the store: tile index y goes to y ^ x.  The thread
  // bits' part moves the lane's base; the register bits' part (tile bits
  // 8..11, uniform) picks each register's row, sixteen scalar offsets.  No
  // work per amplitude.
  {
    const int fx = (fzx >> 16) & (kTile - 1);
    const int xr = fx >> 8;
    double2* dst = A.dst + sbase + octet_spread(M.at(ybase<2>(t) ^ (fx & 255)), og);
#pragma unroll
    for (int r = 0; r < kRegs; ++r) {
      d2v x;
      x.x = v[r].x;
      x.y = v[r].y;
      __builtin_nontemporal_store(x, (d2v*)(dst + octet_spread(M.rel((r ^ xr) << 8), og)));
    }
  }
}

hipError_t launch_wavefront(const WfArgs& a, int kind, hipStream_t stream) {
  if (a.L_eff < kTileBits || a.L_eff > 32 || a.n_steps < 1 || a.n_steps > kWfSteps ||
      a.c < 0 || a.c > kTileBits || a.s < a.c || a.s + kTileBits - a.c > a.L_eff ||
      a.out_bit >= a.L_eff || a.batch < 1 || !a.tab || !a.recs || !a.src || !a.dst)
    return hipErrorInvalidValue;
  if (a.octet_bits && (a.octet_bits < 4 || a.octet_bits > a.L_eff)) return hipErrorInvalidValue;
  // nibble 0's site bits: all four, or only bit 3 when bits 0..2 are columns
  const bool cols3 = a.c == 3;
  if (!cols3 && a.c != kTileBits) return hipErrorInvalidValue;
  for (int st = 0; st < a.n_steps; ++st)
    if (a.mask[st] >> kTileBits || (cols3 && (a.mask[st] & 7u))) return hipErrorInvalidValue;
  // (the frame's Z leaves by the last diagonal: none beyond the trailing one)
  if (a.dmask < 0 || a.dmask >> (a.n_steps + 1)) return hipErrorInvalidValue;
  const int n_tiles = 1 << (a.L_eff - kTileBits);
  const dim3 grid = a.octet_bits ? dim3(n_tiles * 8, (a.batch + 7) / 8) : dim3(n_tiles, a.batch);
  const dim3 block(kThreads);
  constexpr bool kSplit = DTC_WF_SPLIT != 0;
  if (kind == kKindRX) {
    if (cols3) hipLaunchKernelGGL((dtc_wf_pass<kKindRX, 8, kSplit>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((dtc_wf_pass<kKindRX, 15, kSplit>), grid, block, 0, stream, a);
  } else if (kind == kKindRY) {
    if (cols3) hipLaunchKernelGGL((dtc_wf_pass<kKindRY, 8, kSplit>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((dtc_wf_pass<kKindRY, 15, kSplit>), grid, block, 0, stream, a);
  } else {
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace dtc

// Build query (a data symbol, read by tests/test_gpu_wavefront_t1_swap.py): 1
// when tile 1's launches run the swap form
extern "C" __attribute__((visibility("default"))) const int dtc_wf_t1_swap_form =
    (DTC_WF_T1_SWAP != 0 && DTC_WF_SPLIT != 0) ? 1 : 0;
