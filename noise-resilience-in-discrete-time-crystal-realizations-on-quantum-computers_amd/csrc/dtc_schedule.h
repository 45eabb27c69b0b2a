// dtc_schedule.h — the device-free schedule of the engine (dtc_engine.cpp):
// site-group plans, layer chains, passes, and the builders of a batch's launch
// list -- the autocorrelator's (build_autocorr_schedule) with its steps, the
// light-cone ends, the dual fold, the wavefront interior, and the forward
// sweeps' (build_energy_schedule, build_sample_schedule,
// build_prefix_schedule).  Everything here computes with integers
// and opaque buffer addresses: no HIP call, no engine context, so a plain host
// compiler builds it (tools/schedule_check.cpp dumps the schedules it makes,
// tests/test_schedule_cpu.py pins them).  The engine owns the context, the
// buffers, the launches and the results; the wavefront planner stays in
// dtc_wavefront.h.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/dtc.h"
#include "dtc_kernels.h"
#include "dtc_rng.h"
#include "dtc_wavefront.h"
#include "dtc_wf_frame.h"

namespace dtc {
// (hidden: the engine's library exports the C ABI only, as when this code sat
// in the engine's anonymous namespace)
namespace sched __attribute__((visibility("hidden"))) {

struct Group {
  int c, s;  // tile = bits [0, c) + [s, s + tb - c)
  int act;   // active tile-bit mask
  int tb = dtc::kTileBits;  // tile bits: 12, or 13 (the 13-site group, dtc_tile13.hip)
};

struct Plan {
  int L = 0, L_eff = 0, n_chunks = 0, n_tiles = 0, diag_stride = 0;
  int64_t len = 0;
  std::vector<Group> groups;
};

// Site groups: group 0 = sites [0, a0) in a contiguous 4096-amplitude tile;
// further groups take up to `hi_max` sites each (tile = 12 - a column bits of
// >= 128-B rows + the group's sites).  Defaults: 11 + 9 for L = 20.
// Site groups: the low group (tile bits 0..11 = sites 0..a_lo-1) and higher
// groups of a sites each (tile = a_lo.. column bits 0..c-1 + the group's a
// sites, c = 12 - a).  Sizes are chosen so that the register nibble the
// diagonal is applied in never straddles the column boundary c (kernel
// diag_in: one window-table lookup per amplitude): the low group holds 9..12
// sites, a higher group 9, 8 or 4 (c = 3, 4, 8).  Fewest groups first, then
// the largest low group, then the largest higher groups.
// largest_top (sharded states): the high groups in increasing size, so the
// group holding the top bits (the bits an exchange swaps with the rank bits)
// is a large one and the pre-exchange kicks stay below a few free bits of it
// (the slices of dtc_shard_kick_slice).
// split13 (round 6, L = 20 only): a 13-site group at tile bits 0..12
// (dtc_tile13.hip) and a 7-site column group, tile bits 0..4 + sites 13..19
// (pass_body kGeoB7) -- the column pass kicks 7 sites over 512-B runs instead
// of 8 over 256-B runs (tools/tile13_kdk_probe.hip, profiles/r6c_*).
// pl.n_tiles is then the larger group's tile count (buffer sizes); a pass's
// own is 2^(L_eff - tb).
inline Plan make_plan(int L, bool largest_top = false, bool split13 = false) {
  Plan pl;
  pl.L = L;
  pl.L_eff = std::max(L, dtc::kTileBits);
  pl.len = (int64_t)1 << pl.L_eff;
  pl.n_tiles = 1 << (pl.L_eff - dtc::kTileBits);
  pl.n_chunks = (pl.L_eff + dtc::kChunkBits - 1) / dtc::kChunkBits;
  pl.diag_stride = (pl.n_chunks + pl.L_eff) * 64;
  if (split13 && L == 20) {
    pl.groups.push_back(Group{dtc::kMaxTileBits, dtc::kMaxTileBits, (1 << dtc::kMaxTileBits) - 1,
                              dtc::kMaxTileBits});
    pl.groups.push_back(Group{dtc::kB7Cols, dtc::kMaxTileBits, 0xFE0, dtc::kTileBits});
    return pl;
  }
  if (L <= dtc::kTileBits) {
    // one group; the padding sites L..11 get identity kicks (kernel) so the
    // whole 12-bit tile runs the standard round plan
    pl.groups.push_back(Group{0, 0, (1 << dtc::kTileBits) - 1});
    return pl;
  }
  static const int kHi[3] = {9, 8, 4};
  for (int n_hi = (L - dtc::kTileBits + 8) / 9;; ++n_hi) {
    for (int a_lo = dtc::kTileBits; a_lo >= 9; --a_lo) {
      const int need = L - a_lo;
      // n9 nines, n8 eights, the rest fours
      for (int n9 = n_hi; n9 >= 0; --n9) {
        for (int n8 = n_hi - n9; n8 >= 0; --n8) {
          const int n4 = n_hi - n9 - n8;
          if (9 * n9 + 8 * n8 + 4 * n4 != need) continue;
          pl.groups.push_back(Group{0, 0, (1 << a_lo) - 1});
          int s = a_lo;
          for (int kk = 0; kk < 3; ++kk) {
            const int k = largest_top ? 2 - kk : kk;
            const int cnt = k == 0 ? n9 : (k == 1 ? n8 : n4);
            for (int i = 0; i < cnt; ++i) {
              const int a = kHi[k], c = dtc::kTileBits - a;
              pl.groups.push_back(Group{c, s, ((1 << a) - 1) << c});
              s += a;
            }
          }
          return pl;
        }
      }
    }
  }
}

struct RunCfg {
  const dtc_problem* prob;
  Plan pl;
  std::vector<int> row_kind;  // KickKind of every kick-table row
  uint64_t seed;
  int64_t traj_offset;
  int n_traj;
  int noisy;
  uint32_t thr1, thr2, thr3;
  const int* site_of = nullptr;  // device: physical bit -> logical site (shards)
  int octet_bits = 0;            // batch state layout (dtc_kernels.h state_base)
  // sharded state: the tables live in ctx->shard_cache / shard_kick, and a
  // chunk pass covers the low L_eff_override bits of states stride_override apart
  const double2* diag_tab = nullptr;
  const double2* kick_tab = nullptr;
  int L_eff_override = 0;
  int64_t stride_override = 0;
  // device-like noise (dtc_autocorr_device): general non-unitary kicks, no
  // forward pass runs ahead of a branch point (a jump cannot be undone)
  bool device = false;
  std::vector<uint32_t> dev_thr_host;  // [L][3] per-site Pauli thresholds (prep X)
  const uint32_t* dev_thr = nullptr;   // device copies
  const uint32_t* dev_jump = nullptr;
  const double* dev_kraus = nullptr;
  // two-qubit depolarizing noise on the bonds (dtc_autocorr_bond): thresholds of
  // sample_bond per bond (host and device), the instances' angles on the device
  bool bond = false;
  std::vector<uint32_t> bond_thr_host;
  const uint32_t* bond_thr = nullptr;
  const double* bond_h = nullptr;
  const double* bond_phi = nullptr;
};

// The scheduling options, fixed at dtc_open (environment read once there;
// documented test switches).
struct SchedOpts {
  bool lightcone = true;  // DTC_NO_LIGHTCONE unset: light-cone ends of the echo chains
  bool lc_wide = true;    // DTC_NO_LCW unset: five-pass (10-site) light-cone ends
  bool lc_wide3 = true;   // DTC_NO_LCW3 unset: six-pass (12-site) ends where they fit
  bool dual = true;       // DTC_NO_DUAL: echo chains start with a pass of their own
  bool runahead = true;   // DTC_NO_RUNAHEAD: device-noise forward closes periods with K-D
  // Wavefront interior of the echo chains (dtc_wavefront.h, dtc_wavefront.hip):
  // on by default (profiles/r7_wavefront_ab20.txt: C2 +5.4 %);
  // DTC_NO_WAVEFRONT=1 keeps the plain K-D-K interior, DTC_WAVEFRONT=2..4 sets
  // the layer cap per pass (4: the measured best)
  bool wavefront = true;
  int wf_cap = dtc::kWfSteps;
  // DTC_SPLIT13=1: L = 20 sweeps run the 13 / 7 site groups (round 6: built
  // and parity-tested, slower than the 12 / 8 split on the power-capped chip,
  // profiles/r6q_*; the 12 / 8 split stays the default)
  bool split13 = false;
};

// The plan of an autocorrelator sweep (it sizes the buffers, so it is chosen
// before the schedule is built): the 13 / 7 split where its kernels cover
// every pass: L = 20, unitary factored kicks (RX / RY rows), the probe
// measurement only, no prefix -- `plain`: none of device-like noise, bond
// noise, per-site Z, a prefix, the energy echo
inline Plan autocorr_plan(int L, const std::vector<int>& row_kind, const SchedOpts& so,
                          bool plain) {
  bool s13 = so.split13 && L == 20 && plain;
  for (int k : row_kind) s13 = s13 && (k == dtc::kKindRX || k == dtc::kKindRY);
  return make_plan(L, false, s13);
}

// ---- layer chains ---------------------------------------------------------
using dtc::KickDesc;

inline KickDesc no_kick() { return KickDesc{0, 0, 0, 0u, 0u}; }

struct Chain {
  std::vector<KickDesc> X;  // kick layers X_0..X_n
  bool trailing_d = false;  // a D after X_n too
  int diag = dtc::kDiagFwd;
  std::vector<int> kc;      // layers applied per group
  int nd = 0;               // diagonals applied
  bool post_after_d = true; // a pass that applies D may start the next layer
  std::vector<int> prio;    // tie-break between groups with equal kc (lower first); empty = index
  int n() const { return (int)X.size() - 1; }
  int n_d() const { return trailing_d ? n() + 1 : n(); }
  bool done() const {
    if (nd != n_d()) return false;
    for (int k : kc)
      if (k != n() + 1) return false;
    return true;
  }
};

struct PassSpec {
  int group;
  KickDesc pre, post;
  int diag;    // DiagMode
  int d_index; // diagonals applied after this pass (valid when diag)
  // light-cone end of an echo chain (kShapeLC): tile = bits 0..3 + sites
  // lc_w0..lc_w0+7; layers lc[0] D* lc[1] ... D* lc[lc_layers-1] on the window
  // sites of lc_mask (bit 8 l + b: site lc_w0 + b in layer l), then the probe
  int lc_w0 = -1;
  int lc_layers = 0;
  KickDesc lc[dtc::kLcMaxLayers] = {};
  uint64_t lc_mask = 0;
  // the 10-site form (lc_merge_wide): tile bit k = global bit lc_gb[k], lc_mask
  // bit 10 l + k - 2 = tile bit k kicked in layer l
  int lc_wide = 0;
  int8_t lc_gb[dtc::kTileBits] = {};
  // the 12-site form (lc_wide = 2, lc_merge_wide7): tile bit k = global bit
  // j-5+k, bit 12 l + k of the 84-bit mask lc_mask | lc_mask2 << 64
  uint64_t lc_mask2 = 0;
};

// the tile bits a light-cone pass kicks in layer l (nonzero: the layer runs)
inline uint64_t lc_layer_bits(const PassSpec& ps, int l) {
  if (ps.lc_wide == 2) {
    uint64_t m = 0;
    for (int k = 0; k < dtc::kTileBits; ++k) {
      const int bit = 12 * l + k;
      const uint64_t on = bit < 64 ? (ps.lc_mask >> bit) & 1ull : (ps.lc_mask2 >> (bit - 64)) & 1ull;
      m |= on << k;
    }
    return m;
  }
  return ps.lc_wide ? (ps.lc_mask >> (10 * l)) & 0x3FFull
                    : (ps.lc_mask >> (dtc::kLcSites * l)) & 0xFFull;
}

// The tile geometry of a pass (the plan's group, or the light-cone window).
inline Group pass_group(const Plan& pl, const PassSpec& ps) {
  if (ps.lc_w0 >= 0) return Group{4, ps.lc_w0, 0xFF0};
  return pl.groups[ps.group];
}

// Emit the next pass of a chain (greedy, deterministic).
inline PassSpec next_pass(Chain& ch) {
  int G = 0;
  for (int g = 1; g < (int)ch.kc.size(); ++g) {
    const int pg = ch.prio.empty() ? g : ch.prio[g], pG = ch.prio.empty() ? G : ch.prio[G];
    if (ch.kc[g] < ch.kc[G] || (ch.kc[g] == ch.kc[G] && pg < pG)) G = g;
  }
  PassSpec ps{G, no_kick(), no_kick(), dtc::kDiagNone, ch.nd};
  const int n = ch.n();
  if (ch.kc[G] == ch.nd && ch.kc[G] <= n) ps.pre = ch.X[ch.kc[G]++];
  bool level = true;
  for (int k : ch.kc)
    if (k != ch.nd + 1) level = false;
  if (level && ch.nd < ch.n_d()) {
    ps.diag = ch.diag;
    ps.d_index = ++ch.nd;
    if (ch.post_after_d && ch.kc[G] == ch.nd && ch.kc[G] <= n) ps.post = ch.X[ch.kc[G]++];
  }
  return ps;
}

// Shape and matrix family of a pass.
inline int pass_shape(const PassSpec& ps) {
  if (ps.lc_w0 >= 0) return dtc::kShapeLC;
  const bool has_d = ps.diag != dtc::kDiagNone;
  if (ps.pre.enabled && has_d && ps.post.enabled) return dtc::kShapeKDK;
  if (ps.pre.enabled && has_d) return dtc::kShapeKD;
  if (has_d && ps.post.enabled) return dtc::kShapeDK;
  if (ps.pre.enabled && !has_d && !ps.post.enabled) return dtc::kShapeK;
  if (has_d) return dtc::kShapeD;
  return -1;
}

inline int pass_kind(const RunCfg& rc, const PassSpec& ps, int shape) {
  int kind = shape == dtc::kShapeD ? dtc::kKindRX : -1;
  std::vector<const KickDesc*> ks{&ps.pre, &ps.post};
  for (int l = 0; l < ps.lc_layers; ++l)
    if (lc_layer_bits(ps, l)) ks.push_back(&ps.lc[l]);
  for (const KickDesc* k : ks) {
    if (!k->enabled) continue;
    const bool basis_x = k->mode == dtc::kKickBasisX || k->mode == dtc::kKickUndoBasisX;
    int rk = basis_x ? dtc::kKindGen : rc.row_kind[k->row];
    // device-like noise: Kraus x Pauli x gate is not unitary; with one
    // sub-gate per kick it is a real diagonal times a unitary of the family
    // (SiteMat in dtc_kernels.hip: factored, the diagonal deferred); Kraus
    // factors between sub-gates, or a dagger (undo) putting the diagonal on
    // the right, leave only the general form
    if (rc.device && (rk == dtc::kKindRX || rk == dtc::kKindRY)) {
      const bool left_diag = rc.prob->n_sub == 1 && k->mode != dtc::kKickUndo &&
                             k->mode != dtc::kKickUndoBasisX;
      rk = !left_diag ? dtc::kKindGen : (rk == dtc::kKindRX ? dtc::kKindRXU : dtc::kKindRYU);
    }
    kind = (kind < 0 || kind == rk) ? rk : dtc::kKindGen;
  }
  return kind;
}

inline dtc::PassKick pass_kick(const RunCfg& rc, const PassSpec& ps) {
  const Group g = pass_group(rc.pl, ps);
  dtc::PassKick pk{};
  pk.pre = ps.pre;
  pk.post = ps.post;
  pk.lc_layers = ps.lc_layers;
  for (int l = 0; l < dtc::kLcMaxLayers; ++l) pk.lc[l] = ps.lc[l];
  pk.lc_mask = ps.lc_mask;
  pk.lc_mask2 = ps.lc_mask2;
  pk.lc_wide = ps.lc_wide;
  for (int k = 0; k < dtc::kTileBits; ++k) pk.lc_gb[k] = ps.lc_gb[k];
  pk.kind = pass_kind(rc, ps, pass_shape(ps));
  pk.c = g.c;
  pk.s = g.s;
  pk.act = g.act;
  pk.tb = g.tb;
  return pk;
}

// A scheduled pass of a batch (dtc_autocorr builds the whole batch schedule,
// prepares every kick record with one prep launch per segment, then streams
// the passes).
struct Launch {
  PassSpec ps;
  const double2* src;
  double2* dst;
  int meas_mode, meas_at_end, n_obs;
  double* meas_out;
  int64_t meas_stride;
  int no_store = 0;  // the pass's output is never read again (last pass of an echo chain)
  const int64_t* basis = nullptr;  // first pass of a sweep: src = the basis states (synthesised)
  // dual pass (dtc_kdk_dual): ps is a forward K-D-K that also starts an echo
  // chain -- ps2 = {ps's pre-kick, the echo's first kick layer as post}, its
  // tile after the pre-kick, kicked by ps2's post, goes to dst2
  double2* dst2 = nullptr;
  PassSpec ps2{};
  // bond noise: the pass's diagonal is the noisy layer drawn at (bond_stream,
  // bond_counter), of a forward (0) or an inverse (1) period
  int bond_diag = 0;
  uint32_t bond_stream = 0, bond_counter = 0;
  int bond_inv = 0;
  // wavefront pass (dtc_wavefront.hip): wf_steps > 0 kick steps of layers
  // wf_kick[st] on the tile bits wf_mask[st] of tile wf_tile (0: index bits
  // 0..11; 1: three column bits + sites 11..19), partial diagonals per wf_dmask
  // from table set wf_set, kick family wf_kind; ps is unused
  int wf_steps = 0, wf_tile = 0, wf_dmask = 0, wf_set = 0, wf_kind = 0;
  uint32_t wf_mask[dtc::kWfSteps] = {};
  KickDesc wf_kick[dtc::kWfSteps] = {};
  // an end of an energy echo chain (dtc_energy_echo; meas_mode kMeasEnergy,
  // n_obs = 3 L): kPartXEnd -- X of the pass's sites after its last kick,
  // accumulated into the row at energy_row + 2 L -- and, on the chain's last
  // pass, kPartZ at the end of the pass into the row's first 2 L values
  int meas_parts = 0;
  double* energy_row = nullptr;
  // a pass of the forward energy sweep (build_energy_schedule; n_obs = 4 L):
  // kPartZ / kPartXPost go into energy_row, the row of the time the pass's
  // diagonal closes; kPartXPre -- X of the pass's sites at its entry -- into
  // energy_row_pre + 2 L, the row of the time before
  double* energy_row_pre = nullptr;
  // >= 0: after this launch dst holds exactly the state at time t_state (the
  // closing pass of a period in a K-D chain, kd_forward_launches); run_launches
  // then calls the sweep's callback (X-basis rows, sampling)
  int t_state = -1;
};

// The ranges of a measured launch's observables that go into its time rows,
// each accumulated: values [o_first, o_first + n_out) of the pass into out[0 ..
// n_out).  An end of an energy echo chain: the whole row with Z, else its X
// part.  A forward pass: Z, ZZ (with the X taken before the post-kick) into the
// row of its diagonal, the entry X into the row before.
struct ReduceRange {
  double* out;
  int o_first, n_out;
};
inline int reduce_ranges(const Launch& l, int L, ReduceRange out[2]) {
  const int p = l.meas_parts;
  int n = 0;
  if (p & dtc::kPartXEnd) {
    out[n++] = (p & dtc::kPartZ) ? ReduceRange{l.energy_row, 0, 3 * L}
                                 : ReduceRange{l.energy_row + 2 * L, 2 * L, L};
    return n;
  }
  if (p & dtc::kPartZ) out[n++] = ReduceRange{l.energy_row, 0, (p & dtc::kPartXPost) ? 3 * L : 2 * L};
  if (p & dtc::kPartXPre) out[n++] = ReduceRange{l.energy_row_pre + 2 * L, 3 * L, L};
  return n;
}

// The tile geometry of the wavefront tiles (WfArgs / PassKick c, s, act) and
// the index bit outside the tile that one of its bonds reaches.
struct WfGeo {
  int c, s, act, out_bit, site0;  // site0: the site of tile bit c
};
constexpr WfGeo kWfGeo[2] = {{dtc::kTileBits, dtc::kTileBits, 0xFFF, 12, 0}, {3, 11, 0xFF8, 10, 11}};
constexpr int kWfSetStride = (dtc::kWfSteps + 1) * 2 * dtc::kWfTab;  // double2 per instance

// The two standard record rows of a wavefront launch: row j holds steps 2 j
// (pre) and 2 j + 1 (post), each cut to its step's tile bits.
inline dtc::PassKick wf_pass_kick(const Launch& l, int j) {
  const WfGeo& g = kWfGeo[l.wf_tile];
  dtc::PassKick pk{};
  // (every step's layer in lc[], and the launch's program: the Pauli frame of
  // the launch runs across both rows, dtc_wf_frame.h)
  for (int st = 0; st < dtc::kWfSteps; ++st) {
    KickDesc k = no_kick();
    if (st < l.wf_steps && l.wf_mask[st]) {
      k = l.wf_kick[st];
      k.enabled = 1;
      k.skip = (uint32_t)g.act & ~l.wf_mask[st];
    }
    pk.lc[st] = k;
    pk.wf_mask[st] = st < l.wf_steps ? l.wf_mask[st] : 0u;
  }
  pk.pre = pk.lc[2 * j];
  pk.post = pk.lc[2 * j + 1];
  pk.wf_row = 1 + j;
  pk.wf_steps = l.wf_steps;
  pk.wf_dmask = l.wf_dmask;
  pk.kind = l.wf_kind;
  // (tile bit k < 12 = site k for the low tile: c = 12 serves the records too)
  pk.c = g.c;
  pk.s = g.s;
  pk.act = g.act;
  pk.tb = dtc::kTileBits;
  return pk;
}

// Matrix family of each kick-table row: RX if every sub-gate is
// [[real, imag], [imag, real]], RY if every sub-gate is real, else general.
// Both families are closed under products, Paulis and daggers.
inline std::vector<int> classify_rows(const dtc_problem* pr) {
  const int n_rows = std::max(1, pr->T - 1 + pr->t_offset);
  std::vector<int> out(n_rows);
  const size_t per_row = (size_t)pr->L * pr->n_sub;
  for (int r = 0; r < n_rows; ++r) {
    bool rx = true, ry = true;
    for (size_t e = 0; e < per_row; ++e) {
      const double* m = pr->kick + ((size_t)r * per_row + e) * 8;
      // m = {m00.re, m00.im, m01.re, m01.im, m10.re, m10.im, m11.re, m11.im}
      if (!(m[1] == 0.0 && m[2] == 0.0 && m[4] == 0.0 && m[7] == 0.0)) rx = false;
      if (!(m[1] == 0.0 && m[3] == 0.0 && m[5] == 0.0 && m[7] == 0.0)) ry = false;
    }
    out[r] = rx ? dtc::kKindRX : (ry ? dtc::kKindRY : dtc::kKindGen);
  }
  return out;
}

// Forward chain over periods first .. first + n - 1 (rows period-1, RNG counter
// = period, stream `stream`), a diagonal after every layer (fast.py:111-121).
inline Chain forward_chain(const Plan& pl, int first, int n, uint32_t stream) {
  Chain ch;
  for (int k = 0; k < n; ++k)
    ch.X.push_back(KickDesc{1, first + k - 1, dtc::kKickForward, stream, (uint32_t)(first + k)});
  ch.trailing_d = true;
  ch.diag = dtc::kDiagFwd;
  ch.kc.assign(pl.groups.size(), 0);
  return ch;
}

// Echo chain (fast.py:140-143, UF.inverse() per period, periods in reverse):
// D^* K'_p D^* K'_{p-1} ... D^* K'_1, RNG stream `stream`, counter = step k.
// `ahead[g]` marks groups whose state already carries the forward layer
// K_{p+1} (row p): X_0 undoes it exactly before the first D^*.
inline Chain echo_chain(const Plan& pl, int p, uint32_t stream, const std::vector<int>& ahead) {
  Chain ch;
  ch.X.push_back(KickDesc{1, p, dtc::kKickUndo, dtc::kStreamForward, (uint32_t)(p + 1)});
  for (int k = 1; k <= p; ++k)
    ch.X.push_back(KickDesc{1, p - k, dtc::kKickInverse, stream, (uint32_t)k});
  ch.trailing_d = false;
  ch.diag = dtc::kDiagConj;
  ch.kc.resize(pl.groups.size());
  for (size_t g = 0; g < pl.groups.size(); ++g) ch.kc[g] = ahead[g] ? 0 : 1;
  return ch;
}

inline uint64_t group_bits(const Group& g) {
  uint64_t m = 0;
  for (int k = 0; k < g.tb; ++k)
    if (g.act & (1 << k)) m |= 1ull << (k < g.c ? k : g.s + k - g.c);
  return m;
}

// The kick sites of layer `k` in a pass over group g (tile bits outside
// k.skip), below L.
inline uint64_t layer_sites(const Group& g, const KickDesc& k, int L) {
  uint64_t m = 0;
  for (int b = 0; b < g.tb; ++b) {
    if (!(g.act & ~(int)k.skip & (1 << b))) continue;
    const int site = b < g.c ? b : g.s + b - g.c;
    if (site < L) m |= 1ull << site;
  }
  return m;
}

// tile bits of group g that are NOT in mask (left identity by a kick layer)
inline uint32_t skip_bits(const Group& g, uint64_t mask) {
  uint32_t sk = 0;
  for (int k = 0; k < g.tb; ++k) {
    if (!(g.act & (1 << k))) continue;
    const int bit = k < g.c ? k : g.s + k - g.c;
    if (!((mask >> bit) & 1)) sk |= 1u << k;
  }
  return sk;
}

// The kick layers of a chain's last k passes, in order, separated by the
// D*'s (a layer of one period spans two passes: the post-kick of one group and
// the pre-kick of the next); trailing diagonals are dropped.  False when the
// passes do not form such layers (not a D* chain, a light-cone pass already).
inline bool lc_layers_of(const RunCfg& rc, const std::vector<Launch>& sched, int k,
                         std::vector<KickDesc>& desc, std::vector<uint64_t>& sites) {
  const Plan& pl = rc.pl;
  auto same_layer = [](const KickDesc& a, const KickDesc& b) {
    return a.row == b.row && a.mode == b.mode && a.stream == b.stream &&
           a.rng_period == b.rng_period;
  };
  desc.assign(1, no_kick());
  sites.assign(1, 0);
  bool ok = true;
  int pending_d = 0;  // diagonals not yet followed by a kick (trailing ones are dropped)
  auto kick = [&](const Group& g, const KickDesc& kd) {
    for (; pending_d > 0; --pending_d) {
      desc.push_back(no_kick());
      sites.push_back(0);
    }
    if (desc.back().enabled && !same_layer(desc.back(), kd)) ok = false;
    desc.back() = kd;
    desc.back().skip = 0;
    sites.back() |= layer_sites(g, kd, pl.L);
  };
  for (size_t i = sched.size() - k; i < sched.size(); ++i) {
    const PassSpec& ps = sched[i].ps;
    if (ps.lc_w0 >= 0) ok = false;
    if (!ok) break;
    const Group& g = pl.groups[ps.group];
    if (ps.pre.enabled) kick(g, ps.pre);
    if (ps.diag != dtc::kDiagNone) {
      if (ps.diag != dtc::kDiagConj) ok = false;
      ++pending_d;
    }
    if (ps.post.enabled) kick(g, ps.post);
  }
  return ok;
}

// The sites of j's cone (radius r), clipped to [0, L).
inline uint64_t cone_sites(int L, int j, int r) {
  uint64_t cone = 0;
  for (int i = std::max(0, j - r); i <= std::min(L - 1, j + r); ++i) cone |= 1ull << i;
  return cone;
}

// The 10-site light-cone end (dtc_lcw_final): the chain's last five passes
// as six layers r = 5 .. 0 on the window j-5 .. j+4 or j-4 .. j+5 (the cone
// of r = 4 plus the first layer's group), tile bits 0, 1 = global bits 0, 1.
// The kernel's fixed nibble program needs layers r <= 1 on j-2 .. j+1 (nibble
// 1), r <= 3 on nibbles 1 and 2 (+ j+2, j+3, j-4, j-3): checked here, as the
// window's bounds; false leaves the chain to lc_merge's 8-site form.
inline bool lc_merge_wide(const RunCfg& rc, std::vector<Launch>& sched, size_t chain0, int j) {
  const Plan& pl = rc.pl;
  const int L = pl.L;
  if ((int)(sched.size() - chain0) < 5) return false;
  if (j - 4 < 2 || j + 3 > L - 1) return false;
  std::vector<KickDesc> desc;
  std::vector<uint64_t> sites;
  if (!lc_layers_of(rc, sched, 5, desc, sites) || (int)desc.size() != dtc::kLcwLayers) return false;
  uint64_t u = 1ull << j;
  for (int l = 0; l < dtc::kLcwLayers; ++l) {
    sites[l] &= cone_sites(L, j, dtc::kLcwLayers - 1 - l);
    u |= sites[l];
  }
  const uint64_t nib1 = 0xFull << (j - 2);
  const uint64_t nib2 = (3ull << (j + 2)) | (3ull << (j - 4));
  if ((sites[4] | sites[5]) & ~nib1) return false;
  if ((sites[2] | sites[3]) & ~(nib1 | nib2)) return false;
  uint64_t rest = u & ~(nib1 | nib2);
  if (__builtin_popcountll(rest) > 2 || (rest & 3ull)) return false;
  // the two low tile bits beside the columns: the outer sites, padded with
  // free bits of the state (their kicks stay off)
  for (int g = 2; g < pl.L_eff && __builtin_popcountll(rest) < 2; ++g)
    if (!(((nib1 | nib2 | rest) >> g) & 1ull)) rest |= 1ull << g;
  if (__builtin_popcountll(rest) != 2) return false;
  PassSpec lc{sched.back().ps.group, no_kick(), no_kick(), dtc::kDiagConj, sched.back().ps.d_index};
  const int r0 = __builtin_ctzll(rest), r1 = 63 - __builtin_clzll(rest);
  const int gb[dtc::kTileBits] = {0, 1, r0, r1, j - 2, j - 1, j, j + 1, j + 2, j + 3, j - 4, j - 3};
  lc.lc_w0 = j - 4;  // (marks the light-cone pass; the tile is lc_gb)
  lc.lc_wide = 1;
  lc.lc_layers = dtc::kLcwLayers;
  for (int k = 0; k < dtc::kTileBits; ++k) lc.lc_gb[k] = (int8_t)gb[k];
  for (int l = 0; l < dtc::kLcwLayers; ++l) {
    lc.lc[l] = desc[l];
    for (int k = 2; k < dtc::kTileBits; ++k)
      if ((sites[l] >> gb[k]) & 1ull) lc.lc_mask |= 1ull << (10 * l + k - 2);
  }
  const int kind = pass_kind(rc, lc, dtc::kShapeLC);
  if (kind != dtc::kKindRX && kind != dtc::kKindRY) return false;
  const Launch first = sched[sched.size() - 5];
  sched.resize(sched.size() - 5 + 1);
  sched.back() = Launch{lc, first.src, first.dst, dtc::kMeasProbe, 1, 2, nullptr, first.meas_stride};
  return true;
}

// The 12-site light-cone end (dtc_lcw3_final): the chain's last six passes
// as seven layers r = 6 .. 0 on the window j-5 .. j+6, tile bit k = global
// bit j-5+k (no column bits).  The kernel runs a fixed program: layer l may
// kick only sites of its cone that the program visits (l0: j+2 .. j+6 -- the
// C2 chains' first layer is group B's pre-kick; l1: j-5 .. j+5; then the
// cones of radius 4 .. 0); a site the chain leaves unkicked gets the identity
// record.  False leaves the chain to lc_merge_wide.
inline bool lc_merge_wide7(const RunCfg& rc, std::vector<Launch>& sched, size_t chain0, int j) {
  const Plan& pl = rc.pl;
  const int L = pl.L;
  if ((int)(sched.size() - chain0) < 6) return false;
  if (j - 6 < 0 || j + 6 > L - 1 || pl.L_eff != L || pl.L_eff > 32) return false;
  std::vector<KickDesc> desc;
  std::vector<uint64_t> sites;
  if (!lc_layers_of(rc, sched, 6, desc, sites) || (int)desc.size() != dtc::kLcw3Layers) return false;
  auto span = [&](int a, int b) {  // sites j+a .. j+b
    uint64_t m = 0;
    for (int i = j + a; i <= j + b; ++i) m |= 1ull << i;
    return m;
  };
  const uint64_t prog[dtc::kLcw3Layers] = {span(2, 6), span(-5, 5), span(-4, 4), span(-3, 3),
                                           span(-2, 2), span(-1, 1), span(0, 0)};
  for (int l = 0; l < dtc::kLcw3Layers; ++l) {
    sites[l] &= cone_sites(L, j, dtc::kLcw3Layers - 1 - l);
    if (sites[l] & ~prog[l]) return false;
  }
  PassSpec lc{sched.back().ps.group, no_kick(), no_kick(), dtc::kDiagConj, sched.back().ps.d_index};
  lc.lc_w0 = j - 5;  // (marks the light-cone pass; the tile is lc_gb)
  lc.lc_wide = 2;
  lc.lc_layers = dtc::kLcw3Layers;
  for (int k = 0; k < dtc::kTileBits; ++k) lc.lc_gb[k] = (int8_t)(j - 5 + k);
  for (int l = 0; l < dtc::kLcw3Layers; ++l) {
    lc.lc[l] = desc[l];
    for (int k = 0; k < dtc::kTileBits; ++k)
      if ((sites[l] >> (j - 5 + k)) & 1ull) {
        const int bit = 12 * l + k;
        if (bit < 64) lc.lc_mask |= 1ull << bit;
        else lc.lc_mask2 |= 1ull << (bit - 64);
      }
  }
  const int kind = pass_kind(rc, lc, dtc::kShapeLC);
  if (kind != dtc::kKindRX && kind != dtc::kKindRY) return false;
  const Launch first = sched[sched.size() - 6];
  sched.resize(sched.size() - 6 + 1);
  sched.back() = Launch{lc, first.src, first.dst, dtc::kMeasProbe, 1, 2, nullptr, first.meas_stride};
  return true;
}

// Light-cone end of the echo chain sched[chain0 ..) measuring Z_j: replace
// its last k passes by one kShapeLC pass -- six (lc_merge_wide7) or five
// (lc_merge_wide), when enabled and they fit, else k = 4 .. 2 (the first that
// fits) over an 8-site window.
// Layer l of M (r = M - 1 - l diagonals before the probe) only matters on
// sites j-r .. j+r, and the layers' remaining sites must fit the window
// w0 .. w0+7 (4 <= w0 <= L - 8: clear of tile bits 0..3).
inline void lc_merge(const RunCfg& rc, const SchedOpts& so, std::vector<Launch>& sched,
                     size_t chain0, int j) {
  const Plan& pl = rc.pl;
  const int L = pl.L;
  if (so.lc_wide3 && lc_merge_wide7(rc, sched, chain0, j)) return;
  if (so.lc_wide && lc_merge_wide(rc, sched, chain0, j)) return;
  const int n_chain = (int)(sched.size() - chain0);
  for (int k = std::min(4, n_chain); k >= 2; --k) {
    std::vector<KickDesc> desc;
    std::vector<uint64_t> sites;
    const bool ok = lc_layers_of(rc, sched, k, desc, sites);
    const int M = (int)desc.size();
    if (!ok || M > dtc::kLcLayers) continue;
    uint64_t u = 1ull << j;
    for (int l = 0; l < M; ++l) {
      sites[l] &= cone_sites(L, j, M - 1 - l);
      u |= sites[l];
    }
    const int lo = __builtin_ctzll(u), hi = 63 - __builtin_clzll(u);
    const int w0 = std::max(4, std::min(lo, L - 8));
    if (w0 > lo || hi > w0 + 7 || w0 + 8 > pl.L_eff) continue;
    const PassSpec& last = sched.back().ps;
    PassSpec lc{last.group, no_kick(), no_kick(), dtc::kDiagConj, last.d_index};
    lc.lc_w0 = w0;
    lc.lc_layers = M;
    for (int l = 0; l < M; ++l) {
      lc.lc[l] = desc[l];
      lc.lc_mask |= ((sites[l] >> w0) & 0xFFull) << (dtc::kLcSites * l);
    }
    const int kind = pass_kind(rc, lc, dtc::kShapeLC);
    if (kind != dtc::kKindRX && kind != dtc::kKindRY) continue;
    const Launch first = sched[sched.size() - k];
    sched.resize(sched.size() - k + 1);
    sched.back() = Launch{lc, first.src, first.dst, dtc::kMeasProbe, 1, 2, nullptr, first.meas_stride};
    return;
  }
}

// ---- wavefront interior of an echo chain ------------------------------------
// The partial-diagonal table sets of a sweep, one per distinct (tile, factor
// sets of the steps): [set][n_inst][step][outside bit][kWfTab] (WfArgs::tab),
// built on the host as the schedule meets them.
struct WfTables {
  std::vector<std::string> keys;
  std::vector<double> host;  // re, im pairs
  bool dirty = false;
};

// The table set of one planned pass (conjugated factors: the echo's D^*).
inline int wf_table_set(const dtc_problem* pr, const dtc::wf::Pass& ps, bool conj, WfTables& wt) {
  const WfGeo& g = kWfGeo[ps.tile];
  const int L = pr->L;
  std::string key(1, (char)('0' + ps.tile));
  key += conj ? 'c' : 'f';
  for (const dtc::wf::Step& sp : ps.steps) {
    key += sp.kick_mask ? '|' : '/';
    for (const dtc::wf::Factor& f : sp.factors) {
      key += f.bond ? 'b' : 'f';
      key += (char)('A' + f.site);
    }
  }
  for (size_t i = 0; i < wt.keys.size(); ++i)
    if (wt.keys[i] == key) return (int)i;
  const int set = (int)wt.keys.size();
  wt.keys.push_back(key);
  wt.dirty = true;
  const size_t per_set = (size_t)pr->n_inst * kWfSetStride * 2;
  wt.host.resize((size_t)(set + 1) * per_set);
  double* base = wt.host.data() + (size_t)set * per_set;
  for (size_t e = 0; e < per_set; e += 2) {
    base[e] = 1.0;
    base[e + 1] = 0.0;
  }
  auto tile_bit = [&](int site) { return site - g.site0 + (g.c == dtc::kTileBits ? 0 : g.c); };
  auto in_tile = [&](int site) { return site >= g.site0 && tile_bit(site) < dtc::kTileBits; };
  const double sgn = conj ? 0.5 : -0.5;
  // kick steps first, then the trailing kick-less one: table slot st
  int st = 0;
  for (const dtc::wf::Step& sp : ps.steps) {
    const int slot = sp.kick_mask ? st++ : st;
    if (sp.factors.empty()) continue;
    for (int in = 0; in < pr->n_inst; ++in) {
      const double* hh = pr->h + (size_t)in * L;
      const double* pp = pr->phi + (size_t)in * (L - 1);
      for (int var = 0; var < 2; ++var) {
        double* o = base + (((size_t)in * (dtc::kWfSteps + 1) + slot) * 2 + var) * dtc::kWfTab * 2;
        const double zout = var ? -1.0 : 1.0;
        if (dtc::kWfT2Lay1 && g.c == 3 && (slot & 1)) {
          // the column tile's odd slots: its diagonal runs in layout 1, the same
          // factors regrouped into the register table (half 0, over tile bits
          // 3..8) and the thread table (half 1, bits 3, 8..11), dtc_wf_frame.h
          for (int half = 0; half < 2; ++half) {
            const int n_ent = half ? dtc::kWfL1Thr : dtc::kWfL1Reg;
            for (int v = 0; v < n_ent; ++v) {
              auto z = [&](int k) {
                const int pos = half ? dtc::wf_l1_thr_pos(k) : dtc::wf_l1_reg_pos(k);
                return (pos >= 0 && ((v >> pos) & 1)) ? -1.0 : 1.0;
              };
              double ang = 0.0;
              for (const dtc::wf::Factor& f : sp.factors) {
                if (!f.bond) {
                  const int k = tile_bit(f.site);
                  if (dtc::wf_l1_in_reg(k, -1) == (half == 0)) ang += hh[f.site] * z(k);
                } else if (in_tile(f.site) && in_tile(f.site + 1)) {
                  const int k = tile_bit(f.site);
                  if (dtc::wf_l1_in_reg(k, k + 1) == (half == 0)) ang += pp[f.site] * z(k) * z(k + 1);
                } else {
                  const int k = tile_bit(in_tile(f.site) ? f.site : f.site + 1);
                  if (dtc::wf_l1_in_reg(k, -1) == (half == 0)) ang += pp[f.site] * z(k) * zout;
                }
              }
              double* e = o + ((size_t)(half ? dtc::kWfL1Reg : 0) + v) * 2;
              e[0] = std::cos(sgn * ang);
              e[1] = std::sin(sgn * ang);
            }
          }
          continue;
        }
        for (int half = 0; half < 2; ++half) {
          // half 0: index = tile bits 0..6; half 1: tile bits 6..11
          const int bit0 = half ? 6 : 0, n_ent = half ? dtc::kWfTabB : dtc::kWfTabA;
          for (int v = 0; v < n_ent; ++v) {
            auto z = [&](int k) { return ((v >> (k - bit0)) & 1) ? -1.0 : 1.0; };
            double ang = 0.0;
            for (const dtc::wf::Factor& f : sp.factors) {
              if (!f.bond) {
                const int k = tile_bit(f.site);
                if ((k <= 5) == (half == 0)) ang += hh[f.site] * z(k);
              } else if (in_tile(f.site) && in_tile(f.site + 1)) {
                const int k = tile_bit(f.site);
                if ((k <= 5) == (half == 0)) ang += pp[f.site] * z(k) * z(k + 1);
              } else {
                const int k = tile_bit(in_tile(f.site) ? f.site : f.site + 1);
                if ((k <= 5) == (half == 0)) ang += pp[f.site] * z(k) * zout;
              }
            }
            double* e = o + ((size_t)(half ? dtc::kWfTabA : 0) + v) * 2;
            e[0] = std::cos(sgn * ang);
            e[1] = std::sin(sgn * ang);
          }
        }
      }
    }
  }
  return set;
}

// Replace the run of plain stored K-D-K launches sched[r0, r1) of an echo
// chain -- alternating between the two site groups, launch i applying layer i
// as its pre-kick, D^*, layer i + 1 as its post-kick -- by the planner's
// passes over the overlapping tiles.  Leaves the schedule alone (returns
// false) when anything about the run is not the plain pattern.
inline bool wf_replace(const SchedOpts& so, const RunCfg& rc, std::vector<Launch>& sched, size_t r0,
                       size_t r1, WfTables& wt) {
  const int n = (int)(r1 - r0);
  if (n < 3) return false;
  auto same_layer = [](const KickDesc& a, const KickDesc& b) {
    return a.row == b.row && a.mode == b.mode && a.stream == b.stream &&
           a.rng_period == b.rng_period;
  };
  std::vector<KickDesc> layer(n + 1);
  int kind = -1;
  for (int i = 0; i < n; ++i) {
    const Launch& l = sched[r0 + i];
    const PassSpec& ps = l.ps;
    if (pass_shape(ps) != dtc::kShapeKDK || ps.lc_w0 >= 0 || ps.diag != dtc::kDiagConj ||
        ps.pre.mode != dtc::kKickInverse || ps.post.mode != dtc::kKickInverse || ps.pre.skip ||
        ps.post.skip || ps.pre.bond_on || ps.post.bond_on || l.meas_mode != dtc::kMeasNone ||
        l.no_store || l.basis || l.dst2 || l.bond_diag || l.wf_steps || l.src != l.dst ||
        ps.group != (sched[r0].ps.group ^ (i & 1)))
      return false;
    if (i > 0 && !same_layer(sched[r0 + i - 1].ps.post, ps.pre)) return false;
    layer[i] = ps.pre;
    layer[i + 1] = ps.post;
  }
  for (const KickDesc& k : layer) {
    const int rk = rc.row_kind[k.row];
    if (rk != dtc::kKindRX && rk != dtc::kKindRY) return false;
    if (kind >= 0 && rk != kind) return false;  // one kick family per pass
    kind = rk;
  }
  // planner layers 1 .. n + 1 = layer[0 .. n]; the first launch's group is the
  // one behind at entry
  dtc::wf::Problem p = dtc::wf::plain_span(20, 12, 1, sched[r0].ps.group != 0, n);
  p.tiles = {dtc::wf::make_tile(0, 0, 12), dtc::wf::make_tile(3, 11, 9)};
  p.cap = so.wf_cap;
  std::vector<dtc::wf::Pass> plan;
  // a plan must save launches -- except at cap 2 (DTC_WAVEFRONT=2), which lifts
  // a tile's sites by two layers per pass, the plain rate, and never can: that
  // setting only ever is the test switch for the two-step passes, so there a
  // plan of the plain length runs
  if (!dtc::wf::plan(p, plan) || (int)plan.size() > n ||
      ((int)plan.size() == n && so.wf_cap != 2))
    return false;
  std::vector<Launch> out;
  for (const dtc::wf::Pass& ps : plan) {
    Launch l = sched[r0];
    l.ps = PassSpec{ps.tile, no_kick(), no_kick(), dtc::kDiagConj, 0};
    l.wf_tile = ps.tile;
    l.wf_kind = kind;
    l.wf_steps = 0;
    l.wf_dmask = 0;
    for (const dtc::wf::Step& sp : ps.steps) {
      if (!sp.kick_mask) {
        l.wf_dmask |= 1 << l.wf_steps;  // the trailing step
        continue;
      }
      if (l.wf_steps >= dtc::kWfSteps) return false;
      int m = -1;
      for (int k = 0; k < dtc::kTileBits; ++k) {
        if (!((sp.kick_mask >> k) & 1u)) continue;
        if (m >= 0 && sp.layer[k] != m) return false;  // one layer per step (the kernel's records)
        m = sp.layer[k];
      }
      if (m < 1 || m > n + 1) return false;
      if (!sp.factors.empty()) l.wf_dmask |= 1 << l.wf_steps;
      l.wf_mask[l.wf_steps] = sp.kick_mask;
      l.wf_kick[l.wf_steps] = layer[m - 1];
      ++l.wf_steps;
    }
    if (l.wf_steps < 1) return false;  // (a kick-less pass: not planned for these spans)
    l.wf_set = wf_table_set(rc.prob, ps, true, wt);
    out.push_back(l);
  }
  sched.erase(sched.begin() + (std::ptrdiff_t)r0, sched.begin() + (std::ptrdiff_t)r1);
  sched.insert(sched.begin() + (std::ptrdiff_t)r0, out.begin(), out.end());
  return true;
}

// ---- the batch schedule of the autocorrelator --------------------------------
// What a call asks of the schedule, the device addresses its launches record,
// and what the builder reports back.
struct SchedReq {
  bool want_fwd = false, want_echo = false;
  int meas_f = dtc::kMeasProbe, n_obs_f = 2;  // forward measurement: the probe, or per-site Z
  bool energy = false;                        // energy echo (dtc_energy_echo)
  int n_pre = 0;                              // periods of a forward prefix (0: none)
  int octet = 0;                              // the batch's state layout
};
struct SchedBufs {
  const double2* F0;  // what the first forward pass reads (F, or the prefix states)
  double2 *F, *E;
  double *vals_f, *vals_e;
};
struct SchedInfo {
  bool dev_ahead = false;  // device-like noise: the forward runs one kick layer ahead
  int n_folds = 0;         // dual passes
  bool rebuilt = false;    // the run-ahead schedule was given up for K-D forward passes
};

// One build: its inputs, the schedule, and what the steps below share.
struct SchedBuild {
  const RunCfg& rc;
  const SchedOpts& so;
  const SchedReq& rq;
  const SchedBufs& bufs;
  WfTables& wt;
  std::vector<Launch>& sched;
  bool wf_on = false;      // the wavefront interior applies to this sweep
  bool dev_ahead = false;  // device-like noise: the forward runs one kick layer ahead
  bool all_folded = true;  // ... and every chain that had to fold did
  // energy echo: every (t, group) X and every t's Z row assigned exactly once
  std::vector<char> x_done, z_done;
  // device-like noise, K-D forward
  bool dev_kd() const { return rc.device && !dev_ahead; }
};

// wavefront interior of the echo chains: L = 20 in the 12 / 8 plan, unitary
// factored kicks, depolarizing noise only, the probe only, no prefix, the
// octet layout
inline bool wavefront_applies(const RunCfg& rc, const SchedOpts& so, const SchedReq& rq) {
  const Plan& pl = rc.pl;
  bool wf_on = so.wavefront && pl.L == 20 && !rc.device && !rc.bond &&
               rq.meas_f != dtc::kMeasSites && rq.n_pre == 0 && rq.octet > 0 &&
               pl.groups.size() == 2 && pl.groups[0].tb == dtc::kTileBits &&
               pl.groups[0].act == 0xFFF && pl.groups[1].c == 4 && pl.groups[1].s == 12;
  for (int k : rc.row_kind) wf_on = wf_on && (k == dtc::kKindRX || k == dtc::kKindRY);
  return wf_on;
}

// Bond noise: period q's kicks take the outgoing Pauli of layer q - 1 (fw: a
// forward chain whose layer 0 is period `first`'s).
inline void tag_bond(const RunCfg& rc, Chain& fw, int first) {
  if (!rc.bond) return;
  for (size_t k = 1; k < fw.X.size(); ++k) {
    fw.X[k].bond_on = 1u;
    fw.X[k].bond_stream = dtc::kStreamForward;
    fw.X[k].bond_counter = (uint32_t)(first - 1 + k);
  }
}

// ... and a forward pass that applies D takes the per-state tables of the
// noisy layer of period p.
inline void tag_bond_diag(const RunCfg& rc, Launch& l, int p) {
  if (!rc.bond || l.ps.diag == dtc::kDiagNone) return;
  l.bond_diag = 1;
  l.bond_stream = dtc::kStreamForward;
  l.bond_counter = (uint32_t)p;
}

// The sweep's forward chain K_{n_pre+1} D ... K_P D, with its bond tags and the
// order of its groups.
inline Chain sweep_forward_chain(const SchedBuild& b) {
  const RunCfg& rc = b.rc;
  const Plan& pl = rc.pl;
  const dtc_problem* pr = rc.prob;
  const int n_pre = b.rq.n_pre, P = pr->T - 1 + pr->t_offset;
  Chain fw = forward_chain(pl, n_pre + 1, P - n_pre, dtc::kStreamForward);
  fw.post_after_d = !b.dev_kd();
  tag_bond(rc, fw, n_pre + 1);
  // start on a group without the probe site: every echo chain then ends
  // with its kick-only pass on such a group, which the probe does not need
  // (two groups: the closing groups alternate with p, see below)
  fw.prio.resize(pl.groups.size());
  for (size_t g = 0; g < pl.groups.size(); ++g)
    fw.prio[g] = (int)g + (((group_bits(pl.groups[g]) >> pr->probe_site) & 1ull)
                               ? (int)pl.groups.size() : 0);
  return fw;
}

// Step 1: the forward launch of pass ps, closing period p (time t) when it
// applies a diagonal: measured there if wanted, tagged with its noisy layer
// under bond noise.
inline Launch forward_launch(const SchedBuild& b, const PassSpec& ps, int p, int t) {
  const RunCfg& rc = b.rc;
  const dtc_problem* pr = rc.prob;
  const int n_obs_f = b.rq.n_obs_f;
  const bool want_f = b.rq.want_fwd || b.rq.meas_f == dtc::kMeasSites;
  const bool closes = ps.diag != dtc::kDiagNone;
  const bool meas = closes && want_f && t >= 0 && t >= pr->t_first;
  Launch l{ps, b.sched.empty() ? b.bufs.F0 : b.bufs.F, b.bufs.F,
           meas ? b.rq.meas_f : dtc::kMeasNone, 0, n_obs_f,
           meas ? b.bufs.vals_f + (size_t)t * n_obs_f : nullptr, (int64_t)pr->T * n_obs_f};
  tag_bond_diag(rc, l, p);
  return l;
}

// Step 2: the launches of the echo chain at period p (time t), branching off F
// after the forward pass fps; ahead[g]: group g already carries K_{p+1}.
inline const char* echo_chain_launches(SchedBuild& b, const PassSpec& fps, int p, int t,
                                       const std::vector<int>& ahead) {
  const RunCfg& rc = b.rc;
  const Plan& pl = rc.pl;
  const dtc_problem* pr = rc.prob;
  const int T = pr->T, n_v = 3 * pl.L, n_grp = (int)pl.groups.size();
  std::vector<Launch>& sched = b.sched;
  double2* const E = b.bufs.E;
  Chain ec = echo_chain(pl, p, (uint32_t)(1 + t), ahead);
  if (rc.bond) {
    // The echo starts from P_t D'_t ...: on a group that ran ahead, F
    // holds K_{p+1} P_t and X_0's undo (without the Pauli) leaves P_t; on
    // the others X_0 is P_t alone (patched below).  Step k's kicks take
    // the outgoing Pauli of the chain's k-th noisy D^*.
    std::fill(ec.kc.begin(), ec.kc.end(), 0);
    if (pl.groups.size() == 2) {
      // the chain's p + 2 passes alternate between the two groups from its
      // kick-only first pass: start so that the trailing kick-only pass lands
      // on the group without the probe, where it is dropped (below)
      const int gp = ((group_bits(pl.groups[0]) >> pr->probe_site) & 1ull) ? 0 : 1;
      ec.prio.assign(2, 1);
      ec.prio[(p % 2) ? 1 - gp : gp] = 0;
    }
    for (size_t k = 1; k < ec.X.size(); ++k) {
      ec.X[k].bond_on = 1u;
      ec.X[k].bond_stream = (uint32_t)(1 + t);
      ec.X[k].bond_counter = (uint32_t)k;
    }
  }
  if (rc.device && b.so.dual) {
    // device-like noise: the chain starts on the group whose forward
    // K-D closed the period (the dual pass below)
    ec.prio.resize(pl.groups.size());
    for (size_t g = 0; g < pl.groups.size(); ++g)
      ec.prio[g] = (int)g == fps.group ? -1 : (int)g;
  }
  const double2* src = b.bufs.F;
  while (!ec.done()) {
    PassSpec es = next_pass(ec);
    if (rc.bond && es.pre.enabled && es.pre.mode == dtc::kKickUndo && !ahead[es.group]) {
      es.pre.mode = dtc::kKickBondPauli;
      es.pre.row = p - 1;
      es.pre.bond_on = 1u;
      es.pre.bond_stream = dtc::kStreamForward;
      es.pre.bond_counter = (uint32_t)p;
    }
    sched.push_back(Launch{es, src, E, dtc::kMeasNone, 1, 2, nullptr, (int64_t)T * 2});
    if (b.rq.energy && ec.kc[es.group] == ec.n() + 1 && (es.pre.enabled || es.post.enabled)) {
      // the pass that applies the group's last kick layer K'_1 -- the
      // post-kick of a K-D-K / D-K or the kick of a kick-only pass --
      // measures X of the group's sites after it
      const int shp = pass_shape(es);
      const bool last_is_post = shp == dtc::kShapeKDK || shp == dtc::kShapeDK;
      if (!(last_is_post || shp == dtc::kShapeK) || b.x_done[(size_t)t * n_grp + es.group])
        return "internal: dtc_energy_echo: a group ends in another shape";
      b.x_done[(size_t)t * n_grp + es.group] = 1;
      Launch& l = sched.back();
      l.meas_mode = dtc::kMeasEnergy;
      l.meas_at_end = last_is_post ? 1 : 0;  // (a kick-only pass: after its kicks, mid-pass)
      l.n_obs = n_v;
      l.meas_stride = (int64_t)T * n_v;
      l.meas_parts = dtc::kPartXEnd;
      l.energy_row = b.bufs.vals_e + (size_t)t * n_v;
    }
    if (rc.bond && es.diag != dtc::kDiagNone) {
      sched.back().bond_diag = 1;
      sched.back().bond_stream = (uint32_t)(1 + t);
      sched.back().bond_counter = (uint32_t)es.d_index;
      sched.back().bond_inv = 1;
    }
    src = E;
  }
  return nullptr;
}

// Step 3:
// A chain that ends with a kick-only pass on a group without the probe
// site: unitary single-site kicks on other sites leave <Z_j> unchanged
// (K_i^+ Z_j K_i = Z_j), so that pass is dropped and the probe is read
// after the previous one.  Not for device-like noise: its Kraus kicks
// are not unitary and change the trajectory weight.
inline void drop_trailing_kick(SchedBuild& b, size_t chain0) {
  const RunCfg& rc = b.rc;
  std::vector<Launch>& sched = b.sched;
  if (!rc.device && !b.rq.energy && sched.size() - chain0 >= 2) {
    const Launch& l = sched.back();
    const bool kick_only = l.ps.diag == dtc::kDiagNone && !l.ps.post.enabled;
    if (kick_only && !((group_bits(rc.pl.groups[l.ps.group]) >> rc.prob->probe_site) & 1ull))
      sched.pop_back();
  }
}

// Step 4:
// Light cone of <Z_j> through the chain's last kick layers (unitary
// single-site kicks, D diagonal with nearest-neighbour couplings): the
// last layer X_n matters only on j, X_{n-1} on j-1..j+1, X_{n-r} on
// j-r..j+r.  The chain's last k passes (k = 4 .. 2, the most that fit)
// become one measure-only pass over a tile holding the 8-site window
// of the kicks left: their layers, restricted to the cone, with D*
// between them, then the probe.
inline void light_cone_end(SchedBuild& b, size_t chain0) {
  const RunCfg& rc = b.rc;
  // DTC_NO_LIGHTCONE=1: keep the chains' last two passes (development A/B)
  // Bond noise runs the plain chains: the cone tables are per instance, and
  // the dual fold would conjugate the forward layer's table, where the
  // chain's first D^* is a noisy layer of its own
  // The energy echo measures every site: no cone, and the trailing kick-only
  // pass stays (every site's last kick matters)
  const bool lc_enabled = b.so.lightcone && !rc.bond && !b.rq.energy;
  if (!rc.device && lc_enabled && b.sched.size() - chain0 >= 2)
    lc_merge(rc, b.so, b.sched, chain0, rc.prob->probe_site);
}

// Step 5: the chain's last pass measures -- the probe, or the energy echo's
// Z rows -- and stores nothing.
inline const char* mark_chain_end(SchedBuild& b, int t) {
  std::vector<Launch>& sched = b.sched;
  if (b.rq.energy) {
    // the chain's last pass: norm, Z, ZZ of all sites after its kicks
    Launch& l = sched.back();
    if (!(l.meas_parts & dtc::kPartXEnd) || b.z_done[t])
      return "internal: dtc_energy_echo: the chain's last pass ends no group";
    b.z_done[t] = 1;
    l.meas_parts |= dtc::kPartZ;
  } else {
    sched.back().meas_mode = dtc::kMeasProbe;
    sched.back().meas_out = b.bufs.vals_e + (size_t)t * 2;
  }
  // the echo state is only measured: the chain's last pass reads its
  // tiles and stores nothing (the next chain starts from F again)
  sched.back().no_store = 1;
  return nullptr;
}

// May the forward launch f take the echo chain's first launch e as its dual
// branch (step 6)?  F: the forward buffer.
inline bool can_fold(const SchedBuild& b, const Launch& f, const Launch& e) {
  const RunCfg& rc = b.rc;
  const Plan& pl = rc.pl;
  const bool dev_kd = b.dev_kd();
  const int fs = dev_kd ? dtc::kShapeKD : dtc::kShapeKDK;
  const int es = dev_kd ? dtc::kShapeDK : dtc::kShapeKDK;
  // (the dual kernels carry the probe at most: not with per-site Z)
  const bool fok = pass_shape(f.ps) == fs && !f.basis && f.src == b.bufs.F &&
                   pl.groups[f.ps.group].tb == dtc::kTileBits &&
                   (f.meas_mode == dtc::kMeasNone || f.meas_mode == dtc::kMeasProbe);
  const bool eok =
      pass_shape(e.ps) == es && e.ps.lc_w0 < 0 && e.ps.group == f.ps.group &&
      e.ps.post.enabled && !e.meas_parts &&
      (dev_kd ? e.ps.post.skip == 0 && f.ps.pre.skip == 0
              : e.ps.pre.mode == dtc::kKickUndo && e.ps.pre.skip == 0 &&
                    f.ps.post.skip == 0);
  // the fold is exact only when the chain's first pass conjugates the
  // forward's diagonal (one table per instance; d_index only counts
  // each chain's own periods) and, in the unitary case, undoes exactly
  // the forward's post-kick: check it, so a different chain order
  // falls back to the separate passes instead of folding wrongly
  const bool same_d = f.ps.diag == dtc::kDiagFwd && e.ps.diag == dtc::kDiagConj;
  const bool undoes_post =
      dev_kd || (f.ps.post.enabled && f.ps.post.mode == dtc::kKickForward &&
                    e.ps.pre.row == f.ps.post.row &&
                    e.ps.pre.stream == f.ps.post.stream &&
                    e.ps.pre.rng_period == f.ps.post.rng_period);
  const int fk = (fok && same_d && undoes_post) ? pass_kind(rc, f.ps, fs) : -1;
  const bool kind_ok = rc.device ? (fk == dtc::kKindRXU || fk == dtc::kKindRYU ||
                                    fk == dtc::kKindGen)
                                 : (fk == dtc::kKindRX || fk == dtc::kKindRY ||
                                    fk == dtc::kKindGen);
  const PassSpec branch{f.ps.group, f.ps.pre, e.ps.post, dtc::kDiagNone, 0};
  // (run ahead under device-like noise, the chain's first pass holds an
  // undo of a Kraus kick: its own kind is not a factored one, and it
  // never runs)
  return fok && eok && kind_ok && (b.dev_ahead || fk == pass_kind(rc, e.ps, es)) &&
         fk == pass_kind(rc, branch, -1);
}

// Step 6:
// Dual pass: the forward K-D-K on G just before the chain computes
// K_{p+1} D K_p (input); the chain's first pass, on the same G, is
// undo(K_{p+1}) D^* K'_1 of that -- so K'_1 K_p (input), which the
// forward pass forms from its own tile after the pre-kick and stores
// to E: the chain's first read of F and its own pass go away (48 B
// per amplitude instead of 64).  Not when the chain is one pass (the
// light-cone end reads F itself).
// Device-like noise (no forward layer runs ahead): the forward K-D
// on G gives D_p K_p (input), the chain's first pass is D^* K'_1 of
// that on G -- K'_1 K_p (input) again, formed by a K-D dual pass.
// Returns whether the chain's first pass folded.
inline bool dual_fold(SchedBuild& b, size_t chain0) {
  std::vector<Launch>& sched = b.sched;
  // (bond noise: see light_cone_end)
  const bool dual_enabled = b.so.dual && !b.rc.bond;
  if (!(dual_enabled && sched.size() - chain0 >= 2 && chain0 >= 1)) return false;
  Launch& f = sched[chain0 - 1];
  const Launch& e = sched[chain0];
  if (!can_fold(b, f, e)) return false;
  f.ps2 = PassSpec{f.ps.group, f.ps.pre, e.ps.post, dtc::kDiagNone, 0};
  f.dst2 = b.bufs.E;
  sched.erase(sched.begin() + (std::ptrdiff_t)chain0);
  return true;
}

// Step 7:
// Wavefront interior: the run of plain stored K-D-K launches between
// the chain's first pass (here or folded into the forward's dual pass)
// and its end becomes the planner's deeper passes over tiles that
// share site 11 (dtc_wavefront.h): fewer passes over the state
inline void wavefront_interior(SchedBuild& b, size_t chain0) {
  std::vector<Launch>& sched = b.sched;
  if (!(b.wf_on && sched.size() > chain0)) return;
  const bool folded = chain0 >= 1 && sched[chain0 - 1].dst2 == b.bufs.E &&
                      sched[chain0].src == b.bufs.E;
  const size_t r0 = folded ? chain0 : chain0 + 1;
  size_t r1 = sched.size() - 1;  // the chain's end (measure-only)
  // (energy echo: the end is every group's last pass, the run stops
  // before the first of them)
  for (size_t i = chain0; b.rq.energy && i < r1; ++i)
    if (sched[i].meas_parts) r1 = i;
  if (r1 > r0) wf_replace(b.so, b.rc, sched, r0, r1, b.wt);
}

// One pass over the sweep with b.dev_ahead as it stands:
// Forward chain K_1 D K_2 D ... K_P D; after each D_p: measure t = p - t_offset
// and branch the echo at t off F.  The whole batch schedule is built first.
inline const char* build_sweep(SchedBuild& b) {
  const RunCfg& rc = b.rc;
  const Plan& pl = rc.pl;
  const dtc_problem* pr = rc.prob;
  const int n_pre = b.rq.n_pre;
  std::vector<Launch>& sched = b.sched;
  sched.clear();
  b.all_folded = true;
  if (pr->T - 1 + pr->t_offset <= n_pre) return nullptr;
  Chain fw = sweep_forward_chain(b);
  while (!fw.done()) {
    PassSpec ps = next_pass(fw);
    const int p = ps.d_index + n_pre;  // the chain counts its own periods
    const int t = p - pr->t_offset;
    const bool closes = ps.diag != dtc::kDiagNone;
    sched.push_back(forward_launch(b, ps, p, t));
    if (!closes || !b.rq.want_echo || t < 0 || t < pr->t_first) continue;
    std::vector<int> ahead(pl.groups.size());
    for (size_t g = 0; g < pl.groups.size(); ++g) ahead[g] = fw.kc[g] > ps.d_index;
    // run ahead under device-like noise, a chain whose first pass undoes
    // the forward's run-ahead layer must fold (the undo of a Kraus kick
    // cannot run); the sweep's last chain, after a K-D, has none
    bool must_fold = false;
    for (size_t g = 0; g < pl.groups.size(); ++g) must_fold |= b.dev_ahead && ahead[g];
    const size_t chain0 = sched.size();
    if (const char* err = echo_chain_launches(b, ps, p, t, ahead)) return err;
    drop_trailing_kick(b, chain0);
    light_cone_end(b, chain0);
    if (const char* err = mark_chain_end(b, t)) return err;
    if (!dual_fold(b, chain0) && must_fold) b.all_folded = false;
    wavefront_interior(b, chain0);
  }
  return nullptr;
}

// The launches of one batch: null, or the text of an internal error.
// Device-like noise (r5): the forward runs one kick layer ahead, one pass
// per period as in the unitary case, when every echo chain's first pass
// folds into the forward's dual pass -- the chain's echo start is then
// taken before that layer, so the layer (a Kraus kick, not invertible) is
// never undone; if any chain does not fold, the schedule is rebuilt with
// K-D forward passes (two passes per period, nothing run ahead).
inline const char* build_autocorr_schedule(const RunCfg& rc, const SchedOpts& so,
                                           const SchedReq& rq, const SchedBufs& bufs, WfTables& wt,
                                           std::vector<Launch>& sched, SchedInfo& info) {
  const dtc_problem* pr = rc.prob;
  const int T = pr->T, n_grp = (int)rc.pl.groups.size();
  SchedBuild b{rc, so, rq, bufs, wt, sched};
  b.wf_on = wavefront_applies(rc, so, rq);
  b.x_done.assign(rq.energy ? (size_t)T * n_grp : 0, 0);
  b.z_done.assign(rq.energy ? T : 0, 0);
  // (with bond noise: plain chains, K-D forward passes, nothing runs ahead)
  b.dev_ahead = rc.device && so.dual && so.runahead && !rc.bond;
  info = SchedInfo{};
  for (;;) {
    if (const char* err = build_sweep(b)) return err;
    if (!b.dev_ahead || b.all_folded) break;
    b.dev_ahead = false;
    info.rebuilt = true;
  }
  for (int t = std::max(0, pr->t_first); rq.energy && t < T; ++t) {
    if (t + pr->t_offset == 0) continue;
    bool all = b.z_done[t] != 0;
    for (int g = 0; g < n_grp; ++g) all = all && b.x_done[(size_t)t * n_grp + g];
    if (!all) return "internal: dtc_energy_echo left a time row unmeasured";
  }
  info.dev_ahead = b.dev_ahead;
  for (const Launch& l : sched) info.n_folds += l.dst2 != nullptr;
  return nullptr;
}

// ---- the forward sweeps: energy, sampling, the prefix ------------------------
// The launches F -> F of a forward chain from period 1, nothing measured.
inline std::vector<Launch> chain_launches(const RunCfg& rc, Chain fw, double2* F, int n_obs,
                                          int64_t meas_stride) {
  std::vector<Launch> sched;
  while (!fw.done()) {
    Launch l{next_pass(fw), F, F, dtc::kMeasNone, 0, n_obs, nullptr, meas_stride};
    tag_bond_diag(rc, l, l.ps.d_index);
    sched.push_back(l);
  }
  return sched;
}

// The whole forward chain K_1 D ... K_P D in K-D passes (post_after_d = false:
// no pass that applies D starts the next kick layer), so after the pass closing
// period p the state in F is exactly the state at t = p - t_offset: t_state
// there, for t_lo <= t < T.
inline std::vector<Launch> kd_forward_launches(const RunCfg& rc, double2* F, int t_lo, int n_obs,
                                               int64_t meas_stride) {
  const dtc_problem* pr = rc.prob;
  const int P = pr->T - 1 + pr->t_offset;
  if (P <= 0) return {};
  Chain fw = forward_chain(rc.pl, 1, P, dtc::kStreamForward);
  fw.post_after_d = false;
  tag_bond(rc, fw, 1);
  std::vector<Launch> sched = chain_launches(rc, fw, F, n_obs, meas_stride);
  for (Launch& l : sched) {
    const int t = l.ps.d_index - pr->t_offset;
    if (l.ps.diag != dtc::kDiagNone && t >= t_lo && t < pr->T) l.t_state = t;
  }
  return sched;
}

// The energy sweep (dtc_energy*): rows vals[T][3 L] per state -- norm, Z_i |
// Z_i Z_i+1 | X_i -- from passes of 4 L observables (the above mid-pass + X_i
// before the pre-kick).  Null, or the text of an internal error.
//
// The schedule: the forward chain one kick layer past the last period
// (X_P, no D after it), every pass measuring in flight (meas_parts):
//  * a pass closing period p: Z, ZZ after the diagonal and X of its sites
//    before their post-kick X_p -> time p - t_offset;
//  * a pass whose pre-kick is X_nd (nd diagonals applied): X of its sites
//    before that kick -> time nd - t_offset, unless its sites' X at that
//    time is already taken (one group: the post-kick of the previous pass).
// Each group's X at a time is taken exactly once (checked below); the
// reduce accumulates the X ranges into the zeroed per-time rows.
//
// Device-like noise: a non-unitary kick on one site changes <X> of the
// others, so nothing is measured across a kick.  The chain starts no layer
// in a pass that applies D (2 passes per period); after the pass closing
// period p the state is exactly the state at p: Z, ZZ mid-pass, then X by
// one noiseless basis-change pass per site group (E = H^L F; the engine's
// callback at t_state).
//
// Bond noise (dtc_energy_bond): every pass that applies D takes the per-state
// tables of forward layer d_index, and every kick layer after the first the
// outgoing Pauli of the layer before it.  All of the above is measured on
// the state before the outgoing Pauli P_t of layer t + t_offset -- mid-pass
// after D, before the post-kick or the next pass's pre-kick that absorbs
// P_t, and on the X-basis rotation of that same state -- so one sign pass
// over the finished rows (launch_bond_obs_sign) applies P_t to all of them.
inline const char* build_energy_schedule(const RunCfg& rc, double2* F, double* vals,
                                         std::vector<Launch>& sched) {
  const Plan& pl = rc.pl;
  const dtc_problem* pr = rc.prob;
  const int T = pr->T, P = T - 1 + pr->t_offset, G = (int)pl.groups.size();
  const int n_v = 3 * pl.L, n_obs = 4 * pl.L;
  const int64_t stride = (int64_t)T * n_v;
  auto row = [&](int t) { return vals + (size_t)t * n_v; };
  sched.clear();
  if (P <= 0) return nullptr;
  if (rc.device) {
    sched = kd_forward_launches(rc, F, 0, n_obs, stride);
    for (Launch& l : sched)
      if (l.t_state >= 0) {
        l.meas_mode = dtc::kMeasEnergy;
        l.meas_parts = dtc::kPartZ;
        l.energy_row = row(l.t_state);
      }
    return nullptr;
  }
  Chain fw = forward_chain(pl, 1, P + 1, dtc::kStreamForward);
  fw.trailing_d = false;
  fw.X[P].row = P - 1;  // never observed: any valid table row
  tag_bond(rc, fw, 1);
  sched = chain_launches(rc, fw, F, n_obs, stride);
  std::vector<char> x_done((size_t)T * G, 0);
  for (Launch& l : sched) {
    const PassSpec& ps = l.ps;
    const bool closes = ps.diag != dtc::kDiagNone;
    const int g = ps.group, t = ps.d_index - pr->t_offset;
    if (closes && t >= 0 && t < T) {
      l.meas_parts |= dtc::kPartZ;
      l.energy_row = row(t);
      if (ps.post.enabled) {
        l.meas_parts |= dtc::kPartXPost;
        x_done[(size_t)t * G + g] = 1;
      }
    }
    // (nd: the diagonals applied before this pass)
    const int nd = ps.d_index - (closes ? 1 : 0), te = nd - pr->t_offset;
    if (ps.pre.enabled && nd >= 1 && te >= 0 && te < T && !x_done[(size_t)te * G + g]) {
      l.meas_parts |= dtc::kPartXPre;
      l.energy_row_pre = row(te);
      x_done[(size_t)te * G + g] = 1;
    }
    if (l.meas_parts) l.meas_mode = dtc::kMeasEnergy;
  }
  for (int t = 0; t < T; ++t)
    for (int g = 0; g < G; ++g)
      if (t + pr->t_offset >= 1 && !x_done[(size_t)t * G + g])
        return "internal: dtc_energy left an X group unmeasured";
  // the extra kick layer's pass only measures X: its state is never read
  Launch& last = sched.back();
  if (sched.size() >= 2 && pass_shape(last.ps) == dtc::kShapeK &&
      (last.meas_parts & dtc::kPartXPre) && !(last.meas_parts & dtc::kPartZ))
    last.no_store = 1;
  return nullptr;
}

// The sampling sweep (dtc_sample): the K-D chain, every time t_first <= t < T
// past the initial state sampled from the state its closing pass leaves --
// as the energy sweep keeps it under device-like noise, here with the unitary
// kick kinds.
inline std::vector<Launch> build_sample_schedule(const RunCfg& rc, double2* F) {
  return kd_forward_launches(rc, F, rc.prob->t_first, 0, 0);
}

// The forward prefix (dtc_prefix_build): periods 1 .. n_periods in place,
// post_after_d as the autocorrelator's forward chain, so no kick is pending.
inline std::vector<Launch> build_prefix_schedule(const RunCfg& rc, int n_periods, double2* F) {
  Chain fw = forward_chain(rc.pl, 1, n_periods, dtc::kStreamForward);
  fw.post_after_d = !rc.device;
  return chain_launches(rc, fw, F, 2, 0);
}

// ---- the canonical listing of a schedule ------------------------------------
// One line per launch with every field of Launch (tools/schedule_check.cpp,
// and DTC_PRINT_SCHED in development builds).  A pointer prints as the role of
// the buffer it lies in plus its offset in elements, `?` outside every role's
// buffer, `-` when null.
struct DumpRole {
  const char* name;
  const void* base;
  size_t bytes, elem;  // extent, element size
};

inline void dump_ptr(std::FILE* f, const char* key, const void* p,
                     const std::vector<DumpRole>& roles) {
  if (!p) {
    std::fprintf(f, " %s=-", key);
    return;
  }
  for (const DumpRole& r : roles) {
    const char* b = (const char*)r.base;
    if (r.base && (const char*)p >= b && (const char*)p < b + r.bytes) {
      std::fprintf(f, " %s=%s+%zu", key, r.name, (size_t)((const char*)p - b) / r.elem);
      return;
    }
  }
  std::fprintf(f, " %s=?", key);
}

inline void dump_kick(std::FILE* f, const KickDesc& k) {
  // (`-`: every field 0)
  if (!(k.enabled | k.row | k.mode) &&
      !(k.stream | k.rng_period | k.skip | k.bond_on | k.bond_stream | k.bond_counter)) {
    std::fprintf(f, "-");
    return;
  }
  std::fprintf(f, "%d:%d:%d:%u:%u:%x:%u:%u:%u", k.enabled, k.row, k.mode, k.stream, k.rng_period,
               k.skip, k.bond_on, k.bond_stream, k.bond_counter);
}

inline void dump_pass(std::FILE* f, const char* key, const PassSpec& ps) {
  std::fprintf(f, " %s=[g=%d pre=", key, ps.group);
  dump_kick(f, ps.pre);
  std::fprintf(f, " post=");
  dump_kick(f, ps.post);
  std::fprintf(f, " diag=%d d=%d lc_w0=%d lc_layers=%d lc=", ps.diag, ps.d_index, ps.lc_w0,
               ps.lc_layers);
  for (int l = 0; l < dtc::kLcMaxLayers; ++l) {
    if (l) std::fprintf(f, ";");
    dump_kick(f, ps.lc[l]);
  }
  std::fprintf(f, " lc_mask=%llx lc_mask2=%llx lc_wide=%d lc_gb=", (unsigned long long)ps.lc_mask,
               (unsigned long long)ps.lc_mask2, ps.lc_wide);
  for (int k = 0; k < dtc::kTileBits; ++k) std::fprintf(f, k ? ",%d" : "%d", (int)ps.lc_gb[k]);
  std::fprintf(f, "]");
}

inline void dump_schedule(std::FILE* f, const std::vector<Launch>& sched,
                          const std::vector<DumpRole>& roles) {
  for (size_t i = 0; i < sched.size(); ++i) {
    const Launch& l = sched[i];
    std::fprintf(f, "sched %zu shape=%d", i, l.wf_steps ? -2 : pass_shape(l.ps));
    dump_pass(f, "ps", l.ps);
    dump_ptr(f, "src", l.src, roles);
    dump_ptr(f, "dst", l.dst, roles);
    std::fprintf(f, " meas=%d,%d,%d", l.meas_mode, l.meas_at_end, l.n_obs);
    dump_ptr(f, "meas_out", l.meas_out, roles);
    std::fprintf(f, " meas_stride=%lld no_store=%d", (long long)l.meas_stride, l.no_store);
    dump_ptr(f, "basis", l.basis, roles);
    dump_ptr(f, "dst2", l.dst2, roles);
    dump_pass(f, "ps2", l.ps2);
    std::fprintf(f, " bond=%d,%u,%u,%d wf=%d,%d,%x,%d,%d wf_mask=", l.bond_diag, l.bond_stream,
                 l.bond_counter, l.bond_inv, l.wf_steps, l.wf_tile, (unsigned)l.wf_dmask, l.wf_set,
                 l.wf_kind);
    for (int st = 0; st < dtc::kWfSteps; ++st) std::fprintf(f, st ? ",%x" : "%x", l.wf_mask[st]);
    std::fprintf(f, " wf_kick=");
    for (int st = 0; st < dtc::kWfSteps; ++st) {
      if (st) std::fprintf(f, ";");
      dump_kick(f, l.wf_kick[st]);
    }
    std::fprintf(f, " parts=%d", l.meas_parts);
    dump_ptr(f, "energy_row", l.energy_row, roles);
    // (the forward sweeps' fields, only where set: the autocorrelator's listings
    // stay as they were recorded)
    if (l.energy_row_pre) dump_ptr(f, "row_pre", l.energy_row_pre, roles);
    if (l.t_state >= 0) std::fprintf(f, " t_state=%d", l.t_state);
    std::fprintf(f, "\n");
  }
}

}  // namespace sched
}  // namespace dtc
