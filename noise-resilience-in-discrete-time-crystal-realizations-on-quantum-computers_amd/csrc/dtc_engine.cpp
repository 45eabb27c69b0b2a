// dtc_engine.cpp — host-side engine behind the C ABI (include/dtc.h).
//
// Replaces the reference's per-circuit loop
//   for inst: for t in range(T): qc_qiskit(...) -> backend.run(...)
//   (fast.py:217-239, 124-214)
// with one schedule over a batch of state vectors resident in HBM:
//   forward trajectory  F: init -> period 1 -> period 2 -> ...   (measure at each t)
//   echo branch at t    E: F(t) -> U^-1_p ... U^-1_1             (measure at the end)
// so the forward sweep costs T-1+t_offset periods per trajectory instead of
// sum_t t, and each echo point branches off the forward prefix (same
// per-t marginal distribution as the reference's independent circuits).
//
// Both sweeps are "layer chains" X_0 D X_1 D ... (X = a layer of single-site
// kicks, D = the RZZ/RZ diagonal or its conjugate).  The sites are split in
// groups that fit a tile; the scheduler (next_pass) emits passes that each
// finish the pending kick layer on one group, apply D if that completed the
// layer on every group, and start the next layer on the same group.  With two
// groups (L <= 21) every pass applies one D: one HBM round trip per period.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/dtc.h"
#include "dtc_corr.h"
#include "dtc_rdm.h"
#include "dtc_rdm_block.h"
#include "dtc_kernels.h"
#include "dtc_rng.h"
#include "dtc_schedule.h"
#include "dtc_wavefront.h"
#include "dtc_wf_frame.h"

using namespace dtc::sched;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define DTC_HIP(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      return fail(e_ == hipErrorOutOfMemory ? DTC_ENOMEM : DTC_EHIP,                    \
                  std::string(#expr) + ": " + hipGetErrorString(e_));                   \
  } while (0)

#define DTC_TRY(expr)        \
  do {                       \
    int rc_ = (expr);        \
    if (rc_ != DTC_OK) return rc_; \
  } while (0)

struct DevBuf {
  void* p = nullptr;
  size_t n = 0;
};

// Pinned host staging for the per-trajectory results copied back after a
// batch (direct DMA, no zero-filled pageable vector per call).
struct HostBuf {
  double* p = nullptr;
  size_t n = 0;  // doubles
};

struct Pending {
  int kind;
  hipEvent_t e0, e1;
  double bytes;
};

}  // namespace

struct dtc_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  DevBuf F, E, partial, vals_f, vals_e, diag, kick, basis, sitemap;
  DevBuf lc_diag;  // cone diagonals of the light-cone pass, [n_inst][kLcTab]
  DevBuf red_scratch;  // split sums of the two-stage tile reduction (large states)
  DevBuf recs, recs1, pk;               // kick records (batch schedule / single pass), pass list
  DevBuf dev_thr, dev_jump, dev_kraus;  // device-like noise tables (dtc_autocorr_device)
  // bond noise (dtc_autocorr_bond): draw thresholds [L-1], the angles h | phi of
  // every instance, and the current diagonal layer's per-state factor tables
  DevBuf bond_thr, bond_ang, bond_diag;
  // measurement sampling (dtc_sample): the chunk weights of the state being
  // sampled, [batch][n_tiles], and the batch's outcomes, z | x
  DevBuf sample_w, sample_bits;
  // all-pair correlators (dtc_correlations): the chunk partials of the state
  // being measured, [batch][n_tiles][79]
  DevBuf corr_part;
  // reduced density matrices (dtc_rdm): the workgroup partials of the window
  // being measured, [batch][rdm::n_workgroups(L_eff)][512]
  DevBuf rdm_part;
  // block density matrices (dtc_rdm_block_sums): the split partials
  // [batch][n_split][de][de][2], the per-state matrices of the time being
  // measured [batch][d][d][2], and the instance sums of a batch
  // [T][n_blk][instances][d][d][2]
  DevBuf rdmb_part, rdmb_work, rdmb_sum;
  std::vector<dtc::PassKick> pk_host;   // staged pass list (alive until the stream syncs)
  // forward prefix (dtc_prefix_build): every trajectory's state after
  // prefix_periods periods, and what it was built from
  DevBuf prefix;
  std::vector<int64_t> prefix_masks;
  int prefix_periods = -1;  // -1: none
  int64_t prefix_states = 0, prefix_traj_offset = 0, prefix_len = 0;
  int prefix_n_traj = 0, prefix_device = 0;
  uint64_t prefix_hash = 0;
  bool prof = false;
  // options fixed at dtc_open (environment read once there; development A/B
  // switches, documented in DESIGN.md): batch state layout, light-cone pass
  // variant, the basis-synthesising first pass, batch memory budget, verbose
  // batch report; the scheduling options are `so` below
  int octet_bits = 6;        // DTC_OCTET_BITS (0 = contiguous states)
  int lc_split = 1;          // DTC_LC_SPLIT
  int lc_tpb = 0;            // DTC_LC_TPB (0 = default)
  HostBuf host_f, host_e;    // pinned result staging (autocorr / energy)
  uint64_t tables_key = 0;   // upload_tables: the problem whose tables are in place
  bool tables_valid = false;
  // DTC_KDK_SPLIT: which K-D-K passes run three workgroups per CU (dtc_kernels.h
  // PassArgs::kdk_split): the 12-site probe passes, every per-site/energy pass
  int kdk_split = (1 << 7) | (1 << (8 + 7)) | (1 << (8 + 6));
  bool basis_synth = true;   // DTC_NO_BASIS_SYNTH
  double batch_bytes = 0.0;  // DTC_BATCH_BYTES (0 = automatic)
  bool verbose = false;      // DTC_VERBOSE
  int prefix_octet = 0;      // layout the prefix states were built in
  int64_t st_n[DTC_KERNEL_KINDS] = {};
  int64_t lc_launches[4] = {};  // light-cone passes by kernel (dtc_lightcone_counts)
  SchedOpts so;  // the scheduling options (dtc_schedule.h)
  int64_t sched_counts[4] = {};  // dtc_schedule_counts: folds, run-ahead, rebuilt, 13 / 7
  int64_t wf_launches = 0;       // dtc_wavefront_count
  DevBuf wf_tab;                 // the partial-diagonal table sets of the current problem
  double st_ms[DTC_KERNEL_KINDS] = {};
  double st_bytes[DTC_KERNEL_KINDS] = {};
  std::vector<Pending> pending;
  std::vector<hipEvent_t> pool;
  // sharded state (dtc_shard_*): device tables per bit map, cached so that
  // the asynchronous steps of a sweep never re-upload from host memory
  struct ShardTables {
    uint64_t key = 0;
    DevBuf diag;
  };
  std::vector<ShardTables> shard_cache;  // most recent last, at most 4
  std::vector<ShardTables> shard_maps;   // bit -> site maps (diag = the map), at most 4
  DevBuf shard_kick;
  uint64_t shard_kick_key = 0;
};

namespace {

int ensure(DevBuf& b, size_t bytes) {
  if (bytes == 0) bytes = 16;
  if (b.n >= bytes) return DTC_OK;
  if (b.p) {
    (void)hipFree(b.p);
    b.p = nullptr;
    b.n = 0;
  }
  DTC_HIP(hipMalloc(&b.p, bytes));
  b.n = bytes;
  return DTC_OK;
}

int ensure_host(HostBuf& b, size_t n) {
  if (n == 0) n = 1;
  if (b.n >= n) return DTC_OK;
  if (b.p) (void)hipHostFree(b.p);
  b.p = nullptr;
  b.n = 0;
  DTC_HIP(hipHostMalloc((void**)&b.p, n * sizeof(double), hipHostMallocDefault));
  b.n = n;
  return DTC_OK;
}

void release(DevBuf& b) {
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.n = 0;
}

hipEvent_t get_event(dtc_ctx* ctx) {
  if (!ctx->pool.empty()) {
    hipEvent_t e = ctx->pool.back();
    ctx->pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

int resolve_pending(dtc_ctx* ctx) {
  for (auto& p : ctx->pending) {
    float ms = 0.f;
    DTC_HIP(hipEventSynchronize(p.e1));
    DTC_HIP(hipEventElapsedTime(&ms, p.e0, p.e1));
    ctx->st_n[p.kind] += 1;
    ctx->st_ms[p.kind] += ms;
    ctx->st_bytes[p.kind] += p.bytes;
    ctx->pool.push_back(p.e0);
    ctx->pool.push_back(p.e1);
  }
  ctx->pending.clear();
  return DTC_OK;
}

// Profiling: a call leaves its launches' events pending (resolving them costs
// an elapsed-time query per launch while the GPU idles between calls); they
// are resolved by dtc_kernel_stats / dtc_reset_stats, or here once many wait.
int settle_pending(dtc_ctx* ctx) {
  return ctx->pending.size() > 16384 ? resolve_pending(ctx) : DTC_OK;
}

// One launch, bracketed by a pair of events when profiling is on and booked
// under `kind` with its algorithmic bytes (`what`: the launch's text, for the
// error message).
template <class Fn>
int timed(dtc_ctx* ctx, int kind, double bytes, const char* what, Fn&& launch) {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (ctx->prof) {
    e0 = get_event(ctx);
    e1 = get_event(ctx);
    DTC_HIP(hipEventRecord(e0, ctx->stream));
  }
  const hipError_t e = launch();
  if (e != hipSuccess)
    return fail(e == hipErrorOutOfMemory ? DTC_ENOMEM : DTC_EHIP,
                std::string(what) + ": " + hipGetErrorString(e));
  if (ctx->prof) {
    DTC_HIP(hipEventRecord(e1, ctx->stream));
    ctx->pending.push_back(Pending{kind, e0, e1, bytes});
  }
  return DTC_OK;
}
#define DTC_TIMED(ctx, kind, bytes, expr) \
  DTC_TRY(timed(ctx, kind, bytes, #expr, [&] { return (expr); }))

// Diagonal factor tables (RZZ even/odd bonds + RZ, fast.py:115-120):
// D(x) = exp(-i/2 (sum_i h_i z_i + sum_i phi_i z_i z_{i+1})), z_i = 1 - 2 bit_i(x).
// Per instance: n_chunks chunk tables, D(x) = prod_k C_k[(x >> 5k) & 63] (C_k covers
// sites 5k..5k+4 and the bond to site 5k+5 = index bit 5), followed by one window
// table W_g0[v] per start bit g0, v = bits [g0-1, g0+5) of x, holding the terms of
// sites g0..g0+3 and of every bond touching them (the kernel factors
// D(x) = D(x0) / W(x0) * W(x) over the 16 amplitudes of a thread).
double diag_angle(int L, const double* hh, const double* pp, int lo_site, int hi_site,
                  int bond_lo, int bond_hi, int bit0, int v) {
  auto z = [&](int i) -> double { return ((v >> (i - bit0)) & 1) ? -1.0 : 1.0; };
  double ang = 0.0;
  for (int i = lo_site; i < hi_site && i < L; ++i) ang += hh[i] * z(i);
  for (int i = std::max(bond_lo, 0); i < bond_hi && i + 1 < L; ++i) ang += pp[i] * z(i) * z(i + 1);
  return ang;
}

void build_diag_tables(const Plan& pl, int n_inst, const double* h, const double* phi,
                       std::vector<double>& out, const double* const_angle = nullptr) {
  const int L = pl.L;
  out.assign((size_t)n_inst * pl.diag_stride * 2, 0.0);
  for (int in = 0; in < n_inst; ++in) {
    const double* hh = h + (size_t)in * L;
    const double* pp = phi + (size_t)in * (L > 1 ? L - 1 : 0);
    double* o = out.data() + (size_t)in * pl.diag_stride * 2;
    auto put = [&](int e, double ang) {
      o[e * 2] = std::cos(-0.5 * ang);
      o[e * 2 + 1] = std::sin(-0.5 * ang);
    };
    for (int k = 0; k < pl.n_chunks; ++k) {
      const int b0 = dtc::kChunkBits * k;
      const double c0 = (k == 0 && const_angle) ? const_angle[in] : 0.0;
      for (int v = 0; v < 64; ++v)
        put(k * 64 + v, c0 + diag_angle(L, hh, pp, b0, b0 + dtc::kChunkBits, b0,
                                        b0 + dtc::kChunkBits, b0, v));
    }
    for (int g0 = 0; g0 < pl.L_eff; ++g0) {
      for (int v = 0; v < 64; ++v) {
        if (g0 == 0 && (v & 1)) continue;  // bit -1 does not exist
        put((pl.n_chunks + g0) * 64 + v,
            diag_angle(L, hh, pp, g0, g0 + 4, g0 - 1, g0 + 4, g0 - 1, v));
      }
    }
  }
}

dtc::PassArgs base_args(dtc_ctx* ctx, const RunCfg& rc, int64_t batch_start) {
  dtc::PassArgs A{};
  A.state_len = rc.stride_override ? rc.stride_override : rc.pl.len;
  A.L_eff = rc.L_eff_override ? rc.L_eff_override : rc.pl.L_eff;
  A.L_real = rc.pl.L;
  A.batch_start = batch_start;
  A.n_traj = rc.n_traj;
  A.diag = rc.diag_tab ? rc.diag_tab : (const double2*)ctx->diag.p;
  A.n_chunks = rc.pl.n_chunks;
  A.diag_stride = rc.pl.diag_stride;
  A.probe = rc.prob->probe_site;
  A.partial = (double*)ctx->partial.p;
  A.octet_bits = rc.octet_bits;
  A.lc_split = ctx->lc_split;
  A.lc_tpb = ctx->lc_tpb;
  A.kdk_split = ctx->kdk_split;
#ifdef DTC_PHASE_TIMING
  if (const char* e = std::getenv("DTC_DBG_PTR")) A.dbg_ts = (uint64_t*)std::strtoull(e, nullptr, 0);
#endif
  return A;
}

dtc::PrepArgs prep_args(dtc_ctx* ctx, const RunCfg& rc, int64_t batch_start, int batch) {
  dtc::PrepArgs P{};
  P.batch = batch;
  P.batch_start = batch_start;
  P.n_traj = rc.n_traj;
  P.traj_offset = rc.traj_offset;
  P.kick = rc.kick_tab ? rc.kick_tab : (const double2*)ctx->kick.p;
  P.n_sub = rc.prob->n_sub;
  P.L_kick = rc.prob->L;
  P.L_real = rc.pl.L;
  P.site_of = rc.site_of;
  P.thr1 = rc.thr1;
  P.thr2 = rc.thr2;
  P.thr3 = rc.thr3;
  P.seed = rc.seed;
  P.noisy = rc.noisy;
  P.dev_thr = rc.dev_thr;
  P.dev_thr_jump = rc.dev_jump;
  P.dev_kraus = rc.dev_kraus;
  P.bond_thr = rc.bond_thr;
  return P;
}

int launch_reduce_prof(dtc_ctx* ctx, int n_tiles, int n_obs, int batch, double* out,
                       int64_t out_stride, int o_first = 0, int n_out = -1,
                       int accumulate = 0) {
  const int no = n_out < 0 ? n_obs - o_first : n_out;
  double* scratch = nullptr;
  if (dtc::reduce_splits(n_tiles) > 1) {
    // split sums of a large state's tiles ([batch][splits][n_out])
    const size_t need = (size_t)batch * dtc::reduce_splits(n_tiles) * no * sizeof(double);
    if (ctx->red_scratch.n < need) {
      DTC_HIP(hipStreamSynchronize(ctx->stream));  // the previous scratch may be in use
      DTC_TRY(ensure(ctx->red_scratch, need));
    }
    scratch = (double*)ctx->red_scratch.p;
  }
  DTC_TIMED(ctx, DTC_KERNEL_REDUCE, 8.0 * (double)n_tiles * no * batch,
            dtc::launch_reduce((const double*)ctx->partial.p, n_tiles, n_obs, batch, out,
                               out_stride, ctx->stream, o_first, n_out, accumulate, scratch));
  return DTC_OK;
}

// Launch one pass whose kick records are `recs` ([batch][kRecPerState]; null:
// build them first with a one-pass prep launch); if meas_mode != none, reduce
// its observables into meas_out.
int launch_pass_spec(dtc_ctx* ctx, const RunCfg& rc, int64_t batch_start, int batch,
                     const PassSpec& ps, const double2* src, double2* dst, int meas_mode,
                     int meas_at_end, int n_obs, double* meas_out, int64_t meas_stride,
                     const dtc::KickRec* recs = nullptr, int meas_parts = 0,
                     int no_store = 0, const int64_t* basis = nullptr, int swap_k = 0,
                     const dtc::KickRec* recs2 = nullptr, double2* dst2 = nullptr,
                     const double2* state_diag = nullptr) {
  const int shape = pass_shape(ps);
  if (shape < 0) return fail(DTC_EINVAL, "internal: empty pass");
  const int kind = pass_kind(rc, ps, shape);
  if (!recs) {
    DTC_TRY(ensure(ctx->recs1, (size_t)batch * dtc::kRecPerState * sizeof(dtc::KickRec)));
    dtc::PrepArgs P = prep_args(ctx, rc, batch_start, batch);
    P.passes = nullptr;
    P.one = pass_kick(rc, ps);
    P.n_pass = 1;
    P.out = (dtc::KickRec*)ctx->recs1.p;
    DTC_HIP(dtc::launch_prep(P, ctx->stream));
    recs = P.out;
  }
  dtc::PassArgs A = base_args(ctx, rc, batch_start);
  if (state_diag) {
    // bond noise: one table per state of the batch (launch_bond_diag), which
    // the kernels' instance lookup (batch_start + b) / n_traj finds at b
    A.diag = state_diag;
    A.batch_start = 0;
    A.n_traj = 1;
  }
  const Group g = pass_group(rc.pl, ps);
#ifdef DTC_PHASE_TIMING
  if (const char* e = std::getenv("DTC_DBG_GROUP"))
    if (std::atoi(e) != ps.group) A.dbg_ts = nullptr;
#endif
  A.zx_reg = -1;
  A.zx_lane = -1;
  if (meas_mode == dtc::kMeasEnergy) {
    // the layout the kernel measures Z, ZZ in (the pass program's d_lay, or the
    // IO layout at the end): its one bond between a register bit and a lane bit
    const bool pre = shape == dtc::kShapeK || shape == dtc::kShapeKD || shape == dtc::kShapeKDK;
    const bool post = shape == dtc::kShapeDK || shape == dtc::kShapeKDK;
    const dtc::PassProgram pp = dtc::pass_program(dtc::act_nibs(g.act), pre, post);
    // (an energy echo chain's last pass, kPartXEnd: at its end in layout 2)
    const int lay = meas_at_end ? ((meas_parts & dtc::kPartXEnd) ? 2 : pp.IO) : pp.d_lay;
    auto tile_bit = [&](int site) {
      return site < g.c ? site : ((site >= g.s && site < g.s + dtc::kTileBits - g.c) ? g.c + site - g.s : -1);
    };
    for (int i = 0; i + 1 < rc.pl.L; ++i) {
      int reg = -1, lane = -1;
      for (int site : {i, i + 1}) {
        const int tb = tile_bit(site);
        if (tb < 0) continue;
        if (tb >= 4 * lay && tb < 4 * lay + 4) {
          reg = tb - 4 * lay;
        } else {
          const int q = lay == 2 ? tb : (lay == 1 ? (tb < 4 ? tb : tb - 4) : tb - 4);
          if (q < 6) lane = q;
        }
      }
      if (reg >= 0 && lane >= 0) {
        if (A.zx_reg >= 0) return fail(DTC_EINVAL, "internal: two register-lane bonds in one layout");
        A.zx_reg = reg;
        A.zx_lane = lane;
      }
    }
  }
  if (ps.diag != dtc::kDiagNone && g.tb == dtc::kTileBits && g.c != dtc::kB7Cols) {
    // the kernel's diagonal uses the window table of the register nibble it
    // is applied in (the pass program's d_lay; a light-cone pass counts as
    // one with a pre-kick): that nibble must not straddle c
    const bool pre = shape == dtc::kShapeK || shape == dtc::kShapeKD || shape == dtc::kShapeKDK ||
                     shape == dtc::kShapeLC;
    const bool post = shape == dtc::kShapeDK || shape == dtc::kShapeKDK;
    const int tb = 4 * dtc::pass_program(dtc::act_nibs(g.act), pre, post).d_lay;
    if (!(tb >= g.c || tb + 4 <= g.c))
      return fail(DTC_EINVAL, "internal: diagonal nibble straddles the column bits");
  }
  A.src = src;
  A.dst = dst;
  // the source is the basis state (synthesised by the kernel): kick-only passes
  if (basis && shape != dtc::kShapeK) return fail(DTC_EINVAL, "internal: basis source on a non-kick pass");
  A.basis = basis;
  A.c = g.c;
  A.s = g.s;
  A.tile_bits_mid = g.s - g.c;
  A.tile_bits = g.tb;
  A.act = g.act;
  A.recs = recs;
  A.diag_conj = ps.diag == dtc::kDiagConj;
#ifdef DTC_DEV_KNOBS
  // development builds, timing probes only (wrong results): DTC_DBG_CONJ=0 / 1
  // runs every diagonal unconjugated / conjugated
  if (const char* e = std::getenv("DTC_DBG_CONJ")) A.diag_conj = std::atoi(e) != 0;
#endif
  A.meas = meas_mode;
  A.meas_at_end = meas_at_end;
  A.meas_parts = meas_parts;
  A.no_store = no_store;
  A.lc_layers = ps.lc_layers;
  A.lc_mask = ps.lc_mask;
  A.lc_mask2 = ps.lc_mask2;
  A.lc_diag = (const double2*)ctx->lc_diag.p;
  A.lc_wide = ps.lc_wide;
  for (int k = 0; k < dtc::kTileBits; ++k) A.lc_gb[k] = ps.lc_gb[k];
  A.batch = batch;
  A.n_obs = n_obs;
  A.recs2 = recs2;
  A.dst2 = dst2;
  if (dst2 && (!recs2 || (shape != dtc::kShapeKDK && shape != dtc::kShapeKD) || no_store || basis))
    return fail(DTC_EINVAL, "internal: a dual pass is a stored K-D-K / K-D with its branch's records");
  const int kernel = no_store ? DTC_KERNEL_FINAL_PASS
                              : (ps.diag != dtc::kDiagNone ? DTC_KERNEL_LO_PASS : DTC_KERNEL_HI_PASS);
  // the slice's last pre-exchange kick, stored at the partner piece
  if (swap_k > 0 && (shape != dtc::kShapeK || meas_mode != dtc::kMeasNone || basis))
    return fail(DTC_EINVAL, "internal: kick+exchange pass must be a plain kick pass");
  // algorithmic bytes: a read and a store per amplitude, or one of them
  // (measure-only passes store nothing, a basis-synthesising pass reads nothing)
  const double per_amp = (no_store || basis) ? 16.0 : (dst2 ? 48.0 : 32.0);
  int lc_variant = -1;
  DTC_TIMED(ctx, kernel, per_amp * (double)((int64_t)1 << A.L_eff) * batch,
            swap_k > 0 ? dtc::launch_kick_swap(A, swap_k, kind, ctx->stream)
                       : dtc::launch_pass(A, batch, shape, kind, ctx->stream, &lc_variant));
  if (lc_variant >= 0 && lc_variant < 4) ++ctx->lc_launches[lc_variant];
  if (meas_mode != dtc::kMeasNone && meas_out)
    DTC_TRY(launch_reduce_prof(ctx, 1 << (A.L_eff - g.tb), n_obs, batch, meas_out, meas_stride));
  return DTC_OK;
}

int launch_wf(dtc_ctx* ctx, const RunCfg& rc, int64_t batch_start, int batch, const Launch& l,
              const dtc::KickRec* recs) {
  const WfGeo& g = kWfGeo[l.wf_tile];
  dtc::WfArgs A{};
  A.src = l.src;
  A.dst = l.dst;
  A.state_len = rc.pl.len;
  A.L_eff = rc.pl.L_eff;
  A.c = g.c;
  A.s = g.s;
  A.octet_bits = rc.octet_bits;
  A.batch = batch;
  A.batch_start = batch_start;
  A.n_traj = rc.n_traj;
  A.recs = recs;
  A.n_steps = l.wf_steps;
  for (int st = 0; st < dtc::kWfSteps; ++st) A.mask[st] = l.wf_mask[st];
  A.dmask = l.wf_dmask;
  A.tab = (const double2*)ctx->wf_tab.p + (size_t)l.wf_set * rc.prob->n_inst * kWfSetStride;
  A.out_bit = g.out_bit;
  DTC_TIMED(ctx, DTC_KERNEL_LO_PASS, 32.0 * (double)((int64_t)1 << A.L_eff) * batch,
            dtc::launch_wavefront(A, l.wf_kind, ctx->stream));
  ++ctx->wf_launches;
  return DTC_OK;
}

// The per-state diagonal tables of launch l's noisy layer, into ctx->bond_diag
// (one buffer: the stream orders the builder after the pass that read the
// previous layer's tables).
int launch_bond_tables(dtc_ctx* ctx, const RunCfg& rc, int64_t batch_start, int batch,
                       const Launch& l) {
  dtc::BondDiagArgs B{};
  B.out = (double2*)ctx->bond_diag.p;
  B.h = rc.bond_h;
  B.phi = rc.bond_phi;
  B.thr = rc.bond_thr;
  B.L = rc.pl.L;
  B.L_eff = rc.pl.L_eff;
  B.n_chunks = rc.pl.n_chunks;
  B.diag_stride = rc.pl.diag_stride;
  B.batch = batch;
  B.batch_start = batch_start;
  B.n_traj = rc.n_traj;
  B.traj_offset = rc.traj_offset;
  B.seed = rc.seed;
  B.stream = l.bond_stream;
  B.counter = l.bond_counter;
  B.inverse = l.bond_inv;
  if (ctx->bond_diag.n < (size_t)batch * B.diag_stride * sizeof(double2))
    return fail(DTC_EINVAL, "internal: bond table buffer too small");
  DTC_TIMED(ctx, DTC_KERNEL_INIT, (double)batch * B.diag_stride * sizeof(double2),
            dtc::launch_bond_diag(B, ctx->stream));
  return DTC_OK;
}

// The signs of the outgoing Paulis on a batch's finished energy rows
// vals[batch][T][3 L] (dtc_bond.hip bond_obs_sign_kernel), in place.
int launch_bond_signs(dtc_ctx* ctx, const RunCfg& rc, int64_t batch_start, int batch,
                      double* vals, int T) {
  dtc::BondObsArgs B{};
  B.vals = vals;
  B.thr = rc.bond_thr;
  B.L = rc.pl.L;
  B.T = T;
  B.t_offset = rc.prob->t_offset;
  B.batch = batch;
  B.batch_start = batch_start;
  B.n_traj = rc.n_traj;
  B.traj_offset = rc.traj_offset;
  B.seed = rc.seed;
  DTC_TIMED(ctx, DTC_KERNEL_REDUCE, 16.0 * (double)batch * T * 3 * rc.pl.L,
            dtc::launch_bond_obs_sign(B, ctx->stream));
  return DTC_OK;
}

// E = H^L F: one noiseless basis-change pass per site group, F -> E, then
// E -> E.  Each pass prepares its own records in ctx->recs1 (launch_pass_spec),
// so the records of the segment that run_launches is streaming, in ctx->recs,
// stay in place.  measure_last: the last pass leaves per-site Z of E -- X of F
// -- in ctx->partial (1 + L values) for the caller's reduce.
int launch_xbasis(dtc_ctx* ctx, const RunCfg& rc, int64_t batch_start, int batch,
                  const double2* F, double2* E, bool measure_last) {
  const int G = (int)rc.pl.groups.size(), n_obs = measure_last ? 1 + rc.pl.L : 0;
  for (int g = 0; g < G; ++g) {
    PassSpec xs{g, no_kick(), no_kick(), dtc::kDiagNone, 0};
    xs.pre = dtc::KickDesc{1, 0, dtc::kKickBasisX, 0u, 0u, 0u};
    DTC_TRY(launch_pass_spec(ctx, rc, batch_start, batch, xs, g == 0 ? F : E, E,
                             measure_last && g == G - 1 ? dtc::kMeasSites : dtc::kMeasNone,
                             measure_last ? 1 : 0, n_obs, nullptr, 0));
  }
  return DTC_OK;
}

// Stream a batch's schedule: the kick records of every pass prepared with one
// launch per segment, then the passes with their reduces.  `after` (optional):
// called behind a launch, and its reduces, that leaves the state of a time in
// its dst (Launch::t_state >= 0).
using AfterLaunch = std::function<int(const Launch&)>;
int run_launches(dtc_ctx* ctx, const RunCfg& rc, int64_t batch_start, int batch,
                 const std::vector<Launch>& L, const AfterLaunch& after = nullptr) {
#ifdef DTC_DEV_KNOBS
  // development builds: DTC_PRINT_SCHED=1 lists the batch's schedule on stderr
  // (the listing of tools/schedule_check.cpp; F0 there is the prefix here)
  if (std::getenv("DTC_PRINT_SCHED"))
    dump_schedule(stderr, L,
                  {{"F0", ctx->prefix.p, ctx->prefix.n, 16},
                   {"F", ctx->F.p, ctx->F.n, 16},
                   {"E", ctx->E.p, ctx->E.n, 16},
                   {"vals_f", ctx->vals_f.p, ctx->vals_f.n, 8},
                   {"vals_e", ctx->vals_e.p, ctx->vals_e.n, 8},
                   {"basis", ctx->basis.p, ctx->basis.n, 8}});
#endif
  // one record row per launch, two for a dual pass (its echo branch's kicks)
  std::vector<size_t> row0(L.size() + 1);
  ctx->pk_host.clear();
  for (size_t i = 0; i < L.size(); ++i) {
    row0[i] = ctx->pk_host.size();
    if (L[i].wf_steps) {
      ctx->pk_host.push_back(wf_pass_kick(L[i], 0));
      ctx->pk_host.push_back(wf_pass_kick(L[i], 1));
      continue;
    }
    ctx->pk_host.push_back(pass_kick(rc, L[i].ps));
    if (L[i].dst2) ctx->pk_host.push_back(pass_kick(rc, L[i].ps2));
  }
  row0[L.size()] = ctx->pk_host.size();
  const size_t n_rows = ctx->pk_host.size();
  const size_t per_pass = (size_t)batch * dtc::kRecPerState * sizeof(dtc::KickRec);
  // (a pass's records take batch * 27 * 64 B, at most 113 MB at the largest
  // batch of 65535 states, so 256 MiB / per_pass >= 2 always: the lower bound
  // only sizes the buffer of a one-row schedule)
  const size_t seg = std::max<size_t>(2, std::min<size_t>(n_rows, (size_t)(256u << 20) / per_pass));
  DTC_TRY(ensure(ctx->recs, seg * per_pass));
  DTC_TRY(ensure(ctx->pk, n_rows * sizeof(dtc::PassKick)));
  DTC_HIP(hipMemcpyAsync(ctx->pk.p, ctx->pk_host.data(), n_rows * sizeof(dtc::PassKick),
                         hipMemcpyHostToDevice, ctx->stream));
  // segments of whole launches whose rows fit the record buffer
  for (size_t i0 = 0; i0 < L.size();) {
    size_t i1 = i0;
    while (i1 < L.size() && row0[i1 + 1] - row0[i0] <= seg) ++i1;
    dtc::PrepArgs P = prep_args(ctx, rc, batch_start, batch);
    P.passes = (const dtc::PassKick*)ctx->pk.p + row0[i0];
    P.n_pass = (int)(row0[i1] - row0[i0]);
    P.out = (dtc::KickRec*)ctx->recs.p;
    DTC_HIP(dtc::launch_prep(P, ctx->stream));
    for (size_t i = i0; i < i1; ++i) {
      const Launch& l = L[i];
      const dtc::KickRec* rec = P.out + (row0[i] - row0[i0]) * batch * dtc::kRecPerState;
      if (l.wf_steps) {
        DTC_TRY(launch_wf(ctx, rc, batch_start, batch, l, rec));
        continue;
      }
      if (l.bond_diag) DTC_TRY(launch_bond_tables(ctx, rc, batch_start, batch, l));
      DTC_TRY(launch_pass_spec(ctx, rc, batch_start, batch, l.ps, l.src, l.dst, l.meas_mode,
                               l.meas_at_end, l.n_obs, l.meas_out, l.meas_stride, rec,
                               l.meas_parts, l.no_store, l.basis, 0,
                               l.dst2 ? rec + batch * dtc::kRecPerState : nullptr, l.dst2,
                               l.bond_diag ? (const double2*)ctx->bond_diag.p : nullptr));
      // the pass's observables into their (zeroed) time rows (reduce_ranges)
      ReduceRange rr[2];
      const int n_rr = reduce_ranges(l, rc.pl.L, rr);
      for (int k = 0; k < n_rr; ++k)
        DTC_TRY(launch_reduce_prof(ctx, rc.pl.n_tiles, l.n_obs, batch, rr[k].out, l.meas_stride,
                                   rr[k].o_first, rr[k].n_out, 1));
      if (l.t_state >= 0 && after) DTC_TRY(after(l));
    }
    i0 = i1;
  }
  return DTC_OK;
}

// The basis states of a batch (masks already in ctx->basis) as the source of
// its schedule: a first pass that only kicks forms them in registers (no
// zero-fill of F, no read of it); any other first pass reads F, filled here.
int basis_source(dtc_ctx* ctx, std::vector<Launch>& sched, double2* F, int64_t len, int nb,
                 int octet_bits) {
  if (!sched.empty() && pass_shape(sched[0].ps) == dtc::kShapeK && ctx->basis_synth) {
    sched[0].basis = (const int64_t*)ctx->basis.p;
    return DTC_OK;
  }
  DTC_HIP(hipMemsetAsync(F, 0, (size_t)dtc::octet_padded(nb, octet_bits) * len * 16, ctx->stream));
  DTC_HIP(dtc::launch_set_basis(F, len, (const int64_t*)ctx->basis.p, nb, ctx->stream, octet_bits));
  return DTC_OK;
}

// Batch size and state layout of a batched run: B states per launch within
// the memory budget (per_state bytes each), the octet layout (dtc_kernels.h)
// when a batch holds at least one octet; then B is a multiple of 8 unless one
// batch takes every state.
// Batch size and state layout.  The octet layout (eight states interleaved
// at 2^octet_bits amplitudes, one state per XCD) serves states below 1 GiB;
// larger states (L_eff >= 26: C4) stay contiguous, the pass kernels then
// giving each XCD an eighth of a state's tiles (r5r: C4 +3.5 %, the top
// 8-site group's rows 16 MiB apart instead of 128 MiB)
constexpr int kOctetMaxLeff = 25;
void batch_layout(const dtc_ctx* ctx, int L_eff, int64_t S, int64_t& B, int& octet) {
  B = std::min<int64_t>(std::min<int64_t>(B, S), 65535);
  octet = (ctx->octet_bits > 0 && B >= 8 && L_eff <= kOctetMaxLeff) ? ctx->octet_bits : 0;
  if (octet && B < S) B &= ~(int64_t)7;
}

// Run a whole chain; the first pass reads src, every pass writes dst; the
// observables of the final state are reduced into meas_out (if meas_mode).
int run_chain(dtc_ctx* ctx, const RunCfg& rc, int64_t batch_start, int batch, Chain& ch,
              const double2* src, double2* dst, int meas_mode, int n_obs, double* meas_out,
              int64_t meas_stride) {
  const double2* s = src;
  while (!ch.done()) {
    PassSpec ps = next_pass(ch);
    const bool last = ch.done();
    DTC_TRY(launch_pass_spec(ctx, rc, batch_start, batch, ps, s, dst,
                             last ? meas_mode : dtc::kMeasNone, 1, n_obs, meas_out,
                             meas_stride));
    s = dst;
  }
  return DTC_OK;
}

int check_problem(const dtc_problem* pr, const dtc_noise* nz, int max_L = 32) {
  if (!pr || !nz) return fail(DTC_EINVAL, "null problem/noise");
  if (pr->L < 1 || pr->L > max_L)
    return fail(DTC_EINVAL, max_L == 32 ? "L must be in [1, 32] per device (larger: dtc_shard_*)"
                                        : "L out of range");
  if (pr->T < 1) return fail(DTC_EINVAL, "T must be >= 1");
  if (pr->n_inst < 1) return fail(DTC_EINVAL, "n_inst must be >= 1");
  if (pr->probe_site < 0 || pr->probe_site >= pr->L)
    return fail(DTC_EINVAL, "probe_site out of range");
  if (pr->t_offset < 0) return fail(DTC_EINVAL, "t_offset must be >= 0");
  if (pr->t_first < 0 || pr->t_first >= pr->T) return fail(DTC_EINVAL, "t_first out of range");
  if (pr->n_sub < 1 || pr->n_sub > 8) return fail(DTC_EINVAL, "n_sub must be in [1, 8]");
  if (!pr->h || (!pr->phi && pr->L > 1) || !pr->kick)
    return fail(DTC_EINVAL, "null h/phi/kick");
  if (pr->L < 64 && (pr->init_mask >> pr->L) != 0)
    return fail(DTC_EINVAL, "init_mask has bits beyond L");
  if (!(nz->p >= 0.0) || nz->p > 4.0 / 3.0) return fail(DTC_EINVAL, "noise p out of range");
  return DTC_OK;
}

void thresholds(double p, uint32_t* t1, uint32_t* t2, uint32_t* t3) {
  auto thr = [&](int k) -> uint32_t {
    double v = std::floor(k * p / 4.0 * 4294967296.0 + 0.5);
    if (v >= 4294967295.0) v = 4294967295.0;
    if (v < 0) v = 0;
    return (uint32_t)v;
  };
  *t1 = thr(1);
  *t2 = thr(2);
  *t3 = thr(3);
}

// Initial product state of one trajectory: neel X gates (fast.py:127-130)
// followed by their depolarizing draw; X or Y after X returns the site to |0>.
uint64_t init_state_mask(const RunCfg& rc, uint64_t traj) {
  uint64_t m = rc.prob->init_mask;
  if (!rc.noisy) return m;
  for (int i = 0; i < rc.pl.L; ++i) {
    if (!((rc.prob->init_mask >> i) & 1ull)) continue;
    int jump = 0;
    int pz = rc.device ? dtc::sample_device(rc.seed, traj, dtc::kStreamPrep, 0u, (uint32_t)i, 0u,
                                            rc.dev_thr_host.data() + 3 * i, 0u, &jump)
                       : dtc::sample_pauli(rc.seed, traj, dtc::kStreamPrep, 0u, (uint32_t)i, 0u,
                                           rc.thr1, rc.thr2, rc.thr3);
    if (pz == 1 || pz == 2) m &= ~(1ull << i);
  }
  return m;
}

// Cone diagonals of the light-cone pass (dtc_kernels.h, kLcTab): for r = 1..4
// the terms of D on sites j-r+1 .. j+r-1 and every bond touching them, as a
// function of bits lo..hi = j-r .. j+r (clipped to [0, L)); r = 5 split at j
// into bits j-5 .. j (fields j-4 .. j, bonds from j-5) and j .. j+5 (fields
// j+1 .. j+4, bonds from j to j+5).
void build_cone_tables(int L, int j, int n_inst, const double* h, const double* phi,
                       std::vector<double>& out) {
  out.assign((size_t)n_inst * dtc::kLcTab * 2, 0.0);
  for (int in = 0; in < n_inst; ++in) {
    const double* hh = h + (size_t)in * L;
    const double* pp = phi + (size_t)in * (L > 1 ? L - 1 : 0);
    for (int r = 1; r <= 4; ++r) {
      const int lo = std::max(0, j - r), hi = std::min(L - 1, j + r);
      double* o = out.data() + ((size_t)in * dtc::kLcTab + dtc::lc_tab_off(r)) * 2;
      for (int v = 0; v < (1 << (hi - lo + 1)); ++v) {
        const double ang = diag_angle(L, hh, pp, std::max(0, j - r + 1), j + r, j - r, j + r, lo, v);
        const int e = r == 4 ? dtc::lc_pos4(v) : v;  // the radius-4 table's storage swizzle
        o[2 * e] = std::cos(-0.5 * ang);
        o[2 * e + 1] = std::sin(-0.5 * ang);
      }
    }
    for (int part = 0; part < 2; ++part) {
      const int lo = part == 0 ? std::max(0, j - 5) : j;
      const int hi = part == 0 ? j : std::min(L - 1, j + 5);
      double* o = out.data() + ((size_t)in * dtc::kLcTab + (part == 0 ? dtc::kLcTab5a : dtc::kLcTab5b)) * 2;
      for (int v = 0; v < (1 << (hi - lo + 1)); ++v) {
        const double ang = part == 0
                               ? diag_angle(L, hh, pp, std::max(0, j - 4), j + 1, j - 5, j, lo, v)
                               : diag_angle(L, hh, pp, j + 1, j + 5, j, j + 5, lo, v);
        const int e = part == 0 ? dtc::lc_pos5a(v) : v;  // storage swizzle of the j-5 .. j table
        o[2 * e] = std::cos(-0.5 * ang);
        o[2 * e + 1] = std::sin(-0.5 * ang);
      }
    }
    // r = 6 and r = 3 split at j (dtc_lcw3_final; j - 6 >= 0 and j + 6 < L,
    // the only geometry that kernel runs): bits j-6 .. j (fields j-5 .. j,
    // bonds from j-6) and j .. j+6 (fields j+1 .. j+5, bonds up to j+6); bits
    // j-3 .. j and j .. j+3 likewise
    if (j - 6 >= 0 && j + 6 <= L - 1) {
      for (int part = 0; part < 4; ++part) {
        const int off = part == 0 ? dtc::kLcTab6a : part == 1 ? dtc::kLcTab6b
                      : part == 2 ? dtc::kLcTab3a : dtc::kLcTab3b;
        const int r = part < 2 ? 6 : 3;
        double* o = out.data() + ((size_t)in * dtc::kLcTab + off) * 2;
        for (int v = 0; v < (1 << (r + 1)); ++v) {
          const double ang = (part % 2 == 0)
                                 ? diag_angle(L, hh, pp, j - r + 1, j + 1, j - r, j, j - r, v)
                                 : diag_angle(L, hh, pp, j + 1, j + r, j, j + r, j, v);
          o[2 * v] = std::cos(-0.5 * ang);
          o[2 * v + 1] = std::sin(-0.5 * ang);
        }
      }
    }
    // r = 4 split at j (dtc_lcw2_final): the product of the two is the r = 4
    // table (dtc_kernels.h kLcTab4a / kLcTab4b; j - 4 >= 0 and j + 4 < L, the
    // only geometry that kernel runs)
    if (j - 4 >= 0 && j + 4 <= L - 1) {
      for (int part = 0; part < 2; ++part) {
        double* o = out.data() + ((size_t)in * dtc::kLcTab + (part == 0 ? dtc::kLcTab4a : dtc::kLcTab4b)) * 2;
        for (int v = 0; v < 32; ++v) {
          const double ang = part == 0 ? diag_angle(L, hh, pp, j - 3, j + 1, j - 4, j, j - 4, v)
                                       : diag_angle(L, hh, pp, j + 1, j + 4, j, j + 4, j, v);
          o[2 * v] = std::cos(-0.5 * ang);
          o[2 * v + 1] = std::sin(-0.5 * ang);
        }
      }
    }
  }
}

uint64_t fnv(uint64_t h, const void* p, size_t n);

// The problem's device tables (diagonal factors, cone diagonals, kick table),
// uploaded when they differ from the ones in place: a repeated sweep of the
// same problem (the bench's steps, a controller's evaluations) neither
// rebuilds nor re-uploads them, nor waits for the stream.
int upload_tables(dtc_ctx* ctx, const dtc_problem* pr, const Plan& pl) {
  const int n_periods = std::max(1, pr->T - 1 + pr->t_offset);
  const size_t kb = (size_t)n_periods * pr->L * pr->n_sub * 8 * sizeof(double);
  const int32_t shape[6] = {pr->L, pl.L_eff, pr->n_inst, pr->probe_site, n_periods, pr->n_sub};
  uint64_t key = fnv(1469598103934665603ull, shape, sizeof(shape));
  key = fnv(key, pr->h, sizeof(double) * pr->n_inst * pr->L);
  if (pr->L > 1) key = fnv(key, pr->phi, sizeof(double) * pr->n_inst * (pr->L - 1));
  key = fnv(key, pr->kick, kb);
  if (ctx->tables_valid && key == ctx->tables_key) return DTC_OK;
  ctx->tables_valid = false;
  std::vector<double> dt;
  build_diag_tables(pl, pr->n_inst, pr->h, pr->phi, dt);
  DTC_TRY(ensure(ctx->diag, dt.size() * sizeof(double)));
  DTC_HIP(hipMemcpyAsync(ctx->diag.p, dt.data(), dt.size() * sizeof(double),
                         hipMemcpyHostToDevice, ctx->stream));
  if (pr->probe_site >= 0 && pr->probe_site < pr->L) {
    std::vector<double> ct;
    build_cone_tables(pr->L, pr->probe_site, pr->n_inst, pr->h, pr->phi, ct);
    DTC_TRY(ensure(ctx->lc_diag, ct.size() * sizeof(double)));
    DTC_HIP(hipMemcpyAsync(ctx->lc_diag.p, ct.data(), ct.size() * sizeof(double),
                           hipMemcpyHostToDevice, ctx->stream));
  }
  DTC_TRY(ensure(ctx->kick, kb));
  DTC_HIP(hipMemcpyAsync(ctx->kick.p, pr->kick, kb, hipMemcpyHostToDevice, ctx->stream));
  DTC_HIP(hipStreamSynchronize(ctx->stream));
  ctx->tables_key = key;
  ctx->tables_valid = true;
  return DTC_OK;
}

// ---- sharded state (include/dtc.h: dtc_shard) ---------------------------------

int check_shard(const dtc_problem* pr, const dtc_shard* sh) {
  if (!sh) return fail(DTC_EINVAL, "null shard");
  const int L = pr->L, nl = sh->n_local, ng = sh->n_global;
  if (ng < 0 || ng > 16 || nl + ng != L) return fail(DTC_EINVAL, "n_local + n_global must equal L");
  if (nl < dtc::kTileBits || nl > 32) return fail(DTC_EINVAL, "n_local must be in [12, 32]");
  if (sh->n_shards < 1 || sh->first_rank < 0 ||
      (int64_t)sh->first_rank + sh->n_shards > ((int64_t)1 << ng))
    return fail(DTC_EINVAL, "shard ranks outside [0, 2^n_global)");
  std::vector<int> seen(L, 0);
  for (int q = 0; q < L; ++q) {
    const int v = sh->site_of[q];
    if (v < 0 || v >= L || seen[v]++) return fail(DTC_EINVAL, "site_of is not a permutation");
  }
  // every bond between two local sites must join adjacent physical bits
  std::vector<int> bit_of(L);
  for (int q = 0; q < L; ++q) bit_of[sh->site_of[q]] = q;
  for (int i = 0; i + 1 < L; ++i) {
    const int a = bit_of[i], b = bit_of[i + 1];
    if (a < nl && b < nl && std::abs(a - b) != 1)
      return fail(DTC_EINVAL, "a bond between two local sites is not physically adjacent");
  }
  return DTC_OK;
}

// Effective chain of one shard: local fields/bonds over physical bits plus the
// constant angle of the rank's global sites (fields, bonds to and among them).
void shard_chain(const dtc_problem* pr, const dtc_shard* sh, int inst, int rank,
                 double* h_eff, double* phi_eff, double* c_angle) {
  const int L = pr->L, nl = sh->n_local;
  const double* h = pr->h + (size_t)inst * L;
  const double* phi = pr->phi + (size_t)inst * (L > 1 ? L - 1 : 0);
  std::vector<int> bit_of(L);
  for (int q = 0; q < L; ++q) bit_of[sh->site_of[q]] = q;
  auto zg = [&](int site) {  // z of a global site on this rank
    return ((rank >> (bit_of[site] - nl)) & 1) ? -1.0 : 1.0;
  };
  double c = 0.0;
  for (int q = 0; q < nl; ++q) h_eff[q] = h[sh->site_of[q]];
  for (int q = 0; q + 1 < nl; ++q) phi_eff[q] = 0.0;
  for (int i = 0; i < L; ++i)
    if (bit_of[i] >= nl) c += h[i] * zg(i);
  for (int i = 0; i + 1 < L; ++i) {
    const int a = bit_of[i], b = bit_of[i + 1];
    if (a < nl && b < nl) phi_eff[std::min(a, b)] = phi[i];
    else if (a < nl) h_eff[a] += phi[i] * zg(i + 1);
    else if (b < nl) h_eff[b] += phi[i] * zg(i);
    else c += phi[i] * zg(i) * zg(i + 1);
  }
  *c_angle = c;
}

}  // namespace

extern "C" {

const char* dtc_last_error(void) { return g_err.c_str(); }

int32_t dtc_abi_version(void) { return DTC_ABI_VERSION; }

int dtc_open(int32_t device, dtc_ctx** out) {
  if (!out) return fail(DTC_EINVAL, "null out");
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(DTC_ENODEV, "no HIP device");
  if (device < 0 || device >= n) return fail(DTC_EINVAL, "device ordinal out of range");
  hipDeviceProp_t prop;
  DTC_HIP(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(DTC_ENODEV, std::string("libdtc_hip is built for gfx950, device is ") +
                                prop.gcnArchName);
  DTC_HIP(hipSetDevice(device));
  dtc_ctx* c = new dtc_ctx();
  c->device = device;
#ifdef DTC_DEV_KNOBS
  // development A/B builds only (make DEV=1): layout and launch-geometry
  // overrides.  The product library ignores these variables, so a stray one
  // cannot change the HBM layout or the kernels' geometry.
  if (const char* e = std::getenv("DTC_OCTET_BITS")) c->octet_bits = std::atoi(e);
  if (c->octet_bits != 0 && (c->octet_bits < 4 || c->octet_bits > 12)) c->octet_bits = 6;
  if (const char* e = std::getenv("DTC_LC_SPLIT")) c->lc_split = e[0] != '0';
  if (const char* e = std::getenv("DTC_LC_TPB")) c->lc_tpb = std::atoi(e);
  if (const char* e = std::getenv("DTC_KDK_SPLIT")) c->kdk_split = std::atoi(e);
  c->basis_synth = std::getenv("DTC_NO_BASIS_SYNTH") == nullptr;
  if (const char* e = std::getenv("DTC_BATCH_BYTES")) c->batch_bytes = std::atof(e);
#endif
  // documented test switches (the parity tests compare the light-cone ends
  // with the full passes, each form on its own engine)
  c->so.lightcone = std::getenv("DTC_NO_LIGHTCONE") == nullptr;
  c->so.lc_wide = std::getenv("DTC_NO_LCW") == nullptr;
  c->so.lc_wide3 = c->so.lc_wide && std::getenv("DTC_NO_LCW3") == nullptr;
  c->so.dual = std::getenv("DTC_NO_DUAL") == nullptr;
  if (const char* e = std::getenv("DTC_WAVEFRONT")) {
    const int v = std::atoi(e);
    if (v >= 2 && v <= dtc::kWfSteps) c->so.wf_cap = v;
  }
  if (std::getenv("DTC_NO_WAVEFRONT")) c->so.wavefront = false;
  c->so.runahead = std::getenv("DTC_NO_RUNAHEAD") == nullptr;
  if (const char* e = std::getenv("DTC_SPLIT13")) c->so.split13 = std::atoi(e) != 0;
  c->verbose = std::getenv("DTC_VERBOSE") != nullptr;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return fail(DTC_EHIP, "hipStreamCreate failed");
  }
  *out = c;
  return DTC_OK;
}

int dtc_close(dtc_ctx* ctx) {
  if (!ctx) return DTC_OK;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  for (auto& p : ctx->pending) {
    (void)hipEventDestroy(p.e0);
    (void)hipEventDestroy(p.e1);
  }
  for (auto e : ctx->pool) (void)hipEventDestroy(e);
  release(ctx->F);
  release(ctx->E);
  release(ctx->prefix);
  release(ctx->partial);
  release(ctx->vals_f);
  release(ctx->vals_e);
  release(ctx->diag);
  release(ctx->lc_diag);
  release(ctx->wf_tab);
  release(ctx->red_scratch);
  if (ctx->host_f.p) (void)hipHostFree(ctx->host_f.p);
  if (ctx->host_e.p) (void)hipHostFree(ctx->host_e.p);
  release(ctx->kick);
  release(ctx->basis);
  release(ctx->sitemap);
  release(ctx->recs);
  release(ctx->recs1);
  release(ctx->pk);
  release(ctx->bond_diag);
  release(ctx->dev_thr);
  release(ctx->dev_jump);
  release(ctx->dev_kraus);
  release(ctx->bond_thr);
  release(ctx->bond_ang);
  release(ctx->sample_w);
  release(ctx->sample_bits);
  release(ctx->corr_part);
  release(ctx->rdm_part);
  release(ctx->rdmb_part);
  release(ctx->rdmb_work);
  release(ctx->rdmb_sum);
  for (auto& e : ctx->shard_cache) release(e.diag);
  for (auto& e : ctx->shard_maps) release(e.diag);
  release(ctx->shard_kick);
  (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return DTC_OK;
}

int dtc_release_buffers(dtc_ctx* ctx) {
  if (!ctx) return fail(DTC_EINVAL, "null ctx");
  DTC_HIP(hipSetDevice(ctx->device));
  DTC_HIP(hipStreamSynchronize(ctx->stream));
  DTC_TRY(resolve_pending(ctx));
  release(ctx->F);
  release(ctx->E);
  release(ctx->partial);
  release(ctx->red_scratch);
  release(ctx->recs);
  release(ctx->recs1);
  release(ctx->pk);
  release(ctx->bond_diag);
  release(ctx->sample_w);
  release(ctx->sample_bits);
  release(ctx->corr_part);
  release(ctx->rdm_part);
  release(ctx->rdmb_part);
  release(ctx->rdmb_work);
  release(ctx->rdmb_sum);
  return DTC_OK;
}

int dtc_set_profiling(dtc_ctx* ctx, int32_t on) {
  if (!ctx) return fail(DTC_EINVAL, "null ctx");
  ctx->prof = on != 0;
  return DTC_OK;
}

int dtc_reset_stats(dtc_ctx* ctx) {
  if (!ctx) return fail(DTC_EINVAL, "null ctx");
  DTC_TRY(resolve_pending(ctx));
  for (int k = 0; k < DTC_KERNEL_KINDS; ++k) {
    ctx->st_n[k] = 0;
    ctx->st_ms[k] = 0;
    ctx->st_bytes[k] = 0;
  }
  return DTC_OK;
}

int dtc_lightcone_counts(dtc_ctx* ctx, int64_t* counts) {
  if (!ctx || !counts) return fail(DTC_EINVAL, "null ctx / counts");
  for (int k = 0; k < 4; ++k) counts[k] = ctx->lc_launches[k];
  return DTC_OK;
}

int dtc_wavefront_count(dtc_ctx* ctx, int64_t* count) {
  if (!ctx || !count) return fail(DTC_EINVAL, "null argument");
  *count = ctx->wf_launches;
  return DTC_OK;
}

int dtc_schedule_counts(dtc_ctx* ctx, int64_t* counts) {
  if (!ctx || !counts) return fail(DTC_EINVAL, "null ctx / counts");
  for (int k = 0; k < 4; ++k) counts[k] = ctx->sched_counts[k];
  return DTC_OK;
}

int dtc_kernel_stats(dtc_ctx* ctx, int32_t kind, int64_t* launches, double* total_ms,
                     double* total_bytes) {
  if (!ctx || kind < 0 || kind >= DTC_KERNEL_KINDS) return fail(DTC_EINVAL, "bad args");
  DTC_TRY(resolve_pending(ctx));
  if (launches) *launches = ctx->st_n[kind];
  if (total_ms) *total_ms = ctx->st_ms[kind];
  if (total_bytes) *total_bytes = ctx->st_bytes[kind];
  return DTC_OK;
}

int dtc_device_info(dtc_ctx* ctx, char* name, int32_t name_len, int32_t* n_cu,
                    double* hbm_bytes) {
  if (!ctx) return fail(DTC_EINVAL, "null ctx");
  hipDeviceProp_t prop;
  DTC_HIP(hipGetDeviceProperties(&prop, ctx->device));
  if (name && name_len > 0) {
    std::snprintf(name, (size_t)name_len, "%s (%s)", prop.name, prop.gcnArchName);
  }
  if (n_cu) *n_cu = prop.multiProcessorCount;
  if (hbm_bytes) *hbm_bytes = (double)prop.totalGlobalMem;
  return DTC_OK;
}

}  // extern "C"

namespace {

// Host-side tables of dtc_device_noise (see include/dtc.h for the model).
// thr [L][3]: Pauli thresholds of sample_device, jump [L]: its jump threshold,
// kraus [L][3]: a0, a1, b of the weighted amplitude-damping operators.
int device_noise_tables(const dtc_device_noise* dv, int L, std::vector<uint32_t>& thr,
                        std::vector<uint32_t>& jump, std::vector<double>& kraus) {
  if (!dv->p_gate || !dv->t1_us || !dv->t2_us) return fail(DTC_EINVAL, "null device-noise arrays");
  if (!(dv->gate_ns >= 0.0)) return fail(DTC_EINVAL, "gate_ns must be >= 0");
  if (!(dv->readout_p01 >= 0.0 && dv->readout_p01 <= 1.0 && dv->readout_p10 >= 0.0 &&
        dv->readout_p10 <= 1.0))
    return fail(DTC_EINVAL, "read-out errors must be in [0, 1]");
  auto u32 = [](double prob) -> uint32_t {
    double v = std::floor(prob * 4294967296.0 + 0.5);
    if (v >= 4294967295.0) v = 4294967295.0;
    if (v < 0) v = 0;
    return (uint32_t)v;
  };
  jump.assign(L, 0u);
  kraus.assign((size_t)3 * L, 0.0);
  thr.assign((size_t)3 * L, 0u);
  for (int i = 0; i < L; ++i) {
    const double p = dv->p_gate[i];
    if (!(p >= 0.0 && p <= 4.0 / 3.0)) return fail(DTC_EINVAL, "p_gate out of range");
    const double t1 = dv->t1_us[i] > 0.0 ? dv->t1_us[i] * 1e3 : INFINITY;  // ns
    double t2 = dv->t2_us[i] > 0.0 ? dv->t2_us[i] * 1e3 : INFINITY;
    t2 = std::min(t2, 2.0 * t1);
    const double tg = dv->gate_ns;
    const double gamma = std::isinf(t1) ? 0.0 : 1.0 - std::exp(-tg / t1);
    // coherence left by amplitude damping: exp(-tg/(2 T1)); the rest is pure
    // dephasing: Z with probability (1 - r)/2, r = exp(-tg (1/T2 - 1/(2 T1)))
    const double rate = (std::isinf(t2) ? 0.0 : 1.0 / t2) - (std::isinf(t1) ? 0.0 : 0.5 / t1);
    const double pz_deph = 0.5 * (1.0 - std::exp(-tg * std::max(0.0, rate)));
    // dephasing then depolarizing(p): X, Y w.p. p/4, Z w.p. (1-d) p/4 + d (1 - 3p/4)
    const double px = p / 4.0, py = p / 4.0;
    const double pzz = (1.0 - pz_deph) * p / 4.0 + pz_deph * (1.0 - 3.0 * p / 4.0);
    thr[3 * i + 0] = u32(px);
    thr[3 * i + 1] = u32(px + py);
    thr[3 * i + 2] = u32(px + py + pzz);
    const double q1 = gamma / 2.0, q0 = 1.0 - q1;
    jump[i] = u32(q1);
    kraus[3 * i + 0] = 1.0 / std::sqrt(q0);
    kraus[3 * i + 1] = std::sqrt(1.0 - gamma) / std::sqrt(q0);
    kraus[3 * i + 2] = q1 > 0.0 ? std::sqrt(gamma / q1) : 0.0;
  }
  return DTC_OK;
}

int setup_device_noise(dtc_ctx* ctx, const dtc_problem* pr, const dtc_device_noise* dv,
                       RunCfg& rc) {
  std::vector<uint32_t> jump;
  std::vector<double> kraus;
  DTC_TRY(device_noise_tables(dv, pr->L, rc.dev_thr_host, jump, kraus));
  DTC_TRY(ensure(ctx->dev_thr, rc.dev_thr_host.size() * sizeof(uint32_t)));
  DTC_TRY(ensure(ctx->dev_jump, jump.size() * sizeof(uint32_t)));
  DTC_TRY(ensure(ctx->dev_kraus, kraus.size() * sizeof(double)));
  DTC_HIP(hipMemcpyAsync(ctx->dev_thr.p, rc.dev_thr_host.data(),
                         rc.dev_thr_host.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                         ctx->stream));
  DTC_HIP(hipMemcpyAsync(ctx->dev_jump.p, jump.data(), jump.size() * sizeof(uint32_t),
                         hipMemcpyHostToDevice, ctx->stream));
  DTC_HIP(hipMemcpyAsync(ctx->dev_kraus.p, kraus.data(), kraus.size() * sizeof(double),
                         hipMemcpyHostToDevice, ctx->stream));
  DTC_HIP(hipStreamSynchronize(ctx->stream));
  rc.device = true;
  rc.noisy = 1;
  rc.dev_thr = (const uint32_t*)ctx->dev_thr.p;
  rc.dev_jump = (const uint32_t*)ctx->dev_jump.p;
  rc.dev_kraus = (const double*)ctx->dev_kraus.p;
  return DTC_OK;
}

// Thresholds of sample_bond (dtc_rng.h) for p_bond[0 .. L-2]: an error happens
// with probability 15 p / 16.
int bond_thresholds(const dtc_bond_noise* bond, int L, std::vector<uint32_t>& thr) {
  thr.assign(L > 1 ? L - 1 : 0, 0u);
  if (!bond) return DTC_OK;
  if (L > 1 && !bond->p_bond) return fail(DTC_EINVAL, "null p_bond");
  for (int b = 0; b + 1 < L; ++b) {
    const double p = bond->p_bond[b];
    if (!(p >= 0.0 && p <= 16.0 / 15.0)) return fail(DTC_EINVAL, "p_bond must be in [0, 16/15]");
    double v = std::floor(15.0 * p / 16.0 * 4294967296.0 + 0.5);
    if (v >= 4294967295.0) v = 4294967295.0;
    thr[b] = (uint32_t)v;
  }
  return DTC_OK;
}

// Device tables of dtc_bond_noise: the thresholds and the instances' angles
// (the table builder signs them per state, dtc_bond.hip).
int setup_bond_noise(dtc_ctx* ctx, const dtc_problem* pr, const dtc_bond_noise* bond, RunCfg& rc) {
  const int L = pr->L;
  DTC_TRY(bond_thresholds(bond, L, rc.bond_thr_host));
  const size_t nh = (size_t)pr->n_inst * L, np = (size_t)pr->n_inst * (L - 1);
  DTC_TRY(ensure(ctx->bond_thr, rc.bond_thr_host.size() * sizeof(uint32_t)));
  DTC_TRY(ensure(ctx->bond_ang, (nh + np) * sizeof(double)));
  DTC_HIP(hipMemcpyAsync(ctx->bond_thr.p, rc.bond_thr_host.data(),
                         rc.bond_thr_host.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                         ctx->stream));
  DTC_HIP(hipMemcpyAsync(ctx->bond_ang.p, pr->h, nh * sizeof(double), hipMemcpyHostToDevice,
                         ctx->stream));
  DTC_HIP(hipMemcpyAsync((double*)ctx->bond_ang.p + nh, pr->phi, np * sizeof(double),
                         hipMemcpyHostToDevice, ctx->stream));
  DTC_HIP(hipStreamSynchronize(ctx->stream));
  rc.bond = true;
  rc.bond_thr = (const uint32_t*)ctx->bond_thr.p;
  rc.bond_h = (const double*)ctx->bond_ang.p;
  rc.bond_phi = (const double*)ctx->bond_ang.p + nh;
  return DTC_OK;
}

// X content per site of the outgoing Pauli of one noisy diagonal layer: site i
// carries (right part of bond i-1's error) (left part of bond i's error).
uint64_t bond_out_x(const RunCfg& rc, uint64_t traj, uint32_t stream, uint32_t counter) {
  uint64_t m = 0;
  for (int b = 0; b + 1 < rc.pl.L; ++b) {
    const int code = dtc::sample_bond(rc.seed, traj, stream, counter, (uint32_t)b,
                                      rc.bond_thr_host[b]);
    if (dtc::pauli_has_x(code & 3)) m ^= 1ull << b;
    if (dtc::pauli_has_x(code >> 2)) m ^= 1ull << (b + 1);
  }
  return m;
}

// What a prefix must match: the instances' angles and the kick rows of its
// periods (FNV-1a over the bytes), so a continuation inverts the same periods.
uint64_t prefix_hash(const dtc_problem* pr, int n_periods) {
  uint64_t h = 1469598103934665603ull;
  auto mix = [&](const void* p, size_t n) {
    const unsigned char* c = (const unsigned char*)p;
    for (size_t i = 0; i < n; ++i) h = (h ^ c[i]) * 1099511628211ull;
  };
  mix(&pr->L, sizeof(pr->L));
  mix(&pr->n_inst, sizeof(pr->n_inst));
  mix(&pr->n_sub, sizeof(pr->n_sub));
  mix(&pr->init_mask, sizeof(pr->init_mask));
  mix(pr->h, sizeof(double) * (size_t)pr->n_inst * pr->L);
  if (pr->L > 1) mix(pr->phi, sizeof(double) * (size_t)pr->n_inst * (pr->L - 1));
  mix(pr->kick, sizeof(double) * 8 * (size_t)n_periods * pr->L * pr->n_sub);
  return h;
}

// The outputs of dtc_energy_echo / dtc_energy_echo_sums (shapes of dtc_energy /
// dtc_energy_sums): with them autocorr_impl runs its echo sweep with the
// forward unmeasured and every chain ending in the energy measurements.
struct EchoEnergyOut {
  double *z, *zz, *x;
  bool sums;
};

// A batch's finished rows hv[nb][T][3 L] (norm, Z_i | Z_i Z_i+1 | X_i per time)
// into the caller's per-trajectory arrays; the row of the initial time is
// formed from the state's mask.  Rows before t_first (dtc_energy_echo: their
// chains are not built) are left 0.
void energy_rows_out(const dtc_problem* pr, const double* hv, const int64_t* masks, int64_t bs,
                     int nb, int t_first, double* z, double* zz, double* x) {
  const int T = pr->T, L = pr->L, n_v = 3 * L;
  for (int b = 0; b < nb; ++b) {
    const int64_t g = bs + b;
    const uint64_t m = (uint64_t)masks[b];
    for (int t = 0; t < T; ++t) {
      const bool at_init = (t + pr->t_offset == 0), skip = t < t_first;
      const double* vf = hv + ((size_t)b * T + t) * n_v;
      const double* vx = vf + 2 * L - 1;  // X_i at vx[1 + i]
      double* zo = z + ((size_t)g * T + t) * L;
      double* xo = x + ((size_t)g * T + t) * L;
      for (int i = 0; i < L; ++i) {
        zo[i] = skip ? 0.0 : (at_init ? (((m >> i) & 1ull) ? -1.0 : 1.0) : vf[1 + i]);
        xo[i] = (skip || at_init) ? 0.0 : vx[1 + i];
      }
      if (L > 1) {
        double* zzo = zz + ((size_t)g * T + t) * (L - 1);
        for (int i = 0; i + 1 < L; ++i)
          zzo[i] = skip ? 0.0
                        : (at_init ? ((((m >> i) ^ (m >> (i + 1))) & 1ull) ? -1.0 : 1.0)
                                   : vf[1 + L + i]);
      }
    }
  }
}

// The same for the per-instance sums of a batch's rows (traj_sum_kernel),
// hv[instances of the batch][T][3 L], added to the caller's zeroed sums.
void energy_sums_out(const dtc_problem* pr, const double* hv, const int64_t* masks, int64_t bs,
                     int nb, int n_traj, int t_first, double* z, double* zz, double* x) {
  const int T = pr->T, L = pr->L, n_v = 3 * L;
  const int64_t i0 = bs / n_traj, n_ib = (bs + nb - 1) / n_traj - i0 + 1;
  for (int64_t i = 0; i < n_ib; ++i) {
    const int64_t inst = i0 + i;
    for (int t = t_first; t < T; ++t) {
      if (t + pr->t_offset == 0) continue;
      const double* vf = hv + ((size_t)i * T + t) * n_v;
      const double* vx = vf + 2 * L - 1;
      double* zo = z + ((size_t)inst * T + t) * L;
      double* xo = x + ((size_t)inst * T + t) * L;
      for (int k = 0; k < L; ++k) {
        zo[k] += vf[1 + k];
        xo[k] += vx[1 + k];
      }
      if (L > 1) {
        double* zzo = zz + ((size_t)inst * T + t) * (L - 1);
        for (int k = 0; k + 1 < L; ++k) zzo[k] += vf[1 + L + k];
      }
    }
  }
  if (pr->t_offset == 0 && t_first == 0) {
    for (int b = 0; b < nb; ++b) {
      const int64_t inst = (bs + b) / n_traj;
      const uint64_t m = (uint64_t)masks[b];
      double* zo = z + (size_t)inst * T * L;
      for (int k = 0; k < L; ++k) zo[k] += ((m >> k) & 1ull) ? -1.0 : 1.0;
      if (L > 1) {
        double* zzo = zz + (size_t)inst * T * (L - 1);
        for (int k = 0; k + 1 < L; ++k)
          zzo[k] += (((m >> k) ^ (m >> (k + 1))) & 1ull) ? -1.0 : 1.0;
      }
    }
  }
}

// The run configuration of a batched entry point (autocorr, prefix, energy):
// the trajectory checks, the device, the kick rows' families, the plan, the
// depolarizing thresholds, the tables of device-like and bond noise.  plain13:
// the call may run the 13 / 7 split (autocorr_plan, dtc_schedule.h).
int init_run_cfg(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz,
                 const dtc_device_noise* dv, const dtc_bond_noise* bond, uint64_t seed,
                 int64_t traj_offset, int32_t n_traj, bool plain13, RunCfg& rc) {
  if (n_traj < 1) return fail(DTC_EINVAL, "n_traj must be >= 1");
  if (traj_offset < 0) return fail(DTC_EINVAL, "traj_offset must be >= 0");
  DTC_HIP(hipSetDevice(ctx->device));
  rc.prob = pr;
  rc.seed = seed;
  rc.traj_offset = traj_offset;
  rc.n_traj = n_traj;
  rc.noisy = nz->p > 0.0 ? 1 : 0;
  rc.row_kind = classify_rows(pr);
  rc.pl = autocorr_plan(pr->L, rc.row_kind, ctx->so, plain13);
  thresholds(nz->p, &rc.thr1, &rc.thr2, &rc.thr3);
  if (dv) DTC_TRY(setup_device_noise(ctx, pr, dv, rc));
  if (bond) DTC_TRY(setup_bond_noise(ctx, pr, bond, rc));
  return DTC_OK;
}

// Automatic batch size: states of per_state bytes within a share of the free
// memory plus `reusable` (the batch buffers this call may reuse or regrow).
// Small states: ~64 GiB of batch saturates the device; with large_state_rule
// (the autocorrelator), large states (L >= 24, C4-style instance batches) may
// use most of the 288 GB, and DTC_BATCH_BYTES (development builds) sets the
// budget.
int auto_batch(dtc_ctx* ctx, double per_state, size_t reusable, bool large_state_rule,
               int64_t& B) {
  size_t free_b = 0, total_b = 0;
  DTC_HIP(hipMemGetInfo(&free_b, &total_b));
  free_b += reusable;
  double budget = (large_state_rule && per_state >= (double)(256ull << 20))
                      ? 0.7 * (double)free_b
                      : std::min(0.6 * (double)free_b, 64.0 * (1ull << 30));
  if (large_state_rule && ctx->batch_bytes > 0) budget = ctx->batch_bytes;
  B = (int64_t)(budget / per_state);
  B = std::max<int64_t>(1, std::min<int64_t>(B, 4096));
  return DTC_OK;
}

// The batches of a batched run: S states, B per batch (Bp: padded to whole
// octets), in the state layout `octet` (dtc_kernels.h state_base).
struct Batch {
  int64_t S = 0, B = 0, Bp = 0;
  int octet = 0;
};

// Size a run's batches and make room for one: the problem's batch size, or the
// automatic one (auto_batch: states of per_state bytes, `reusable`, the
// large-state rule), capped at max_B where given (> 0); its layout, into rc
// too; then F, E (need_E) and the basis masks.  prefix_octet >= 0: the states
// the run starts from are in place in that layout (dtc_prefix_build), which
// the batches take over.
int plan_batch(dtc_ctx* ctx, RunCfg& rc, double per_state, size_t reusable, bool large_state_rule,
               int64_t max_B, bool need_E, int prefix_octet, Batch& bt) {
  bt.S = (int64_t)rc.prob->n_inst * rc.n_traj;
  bt.B = rc.prob->batch;
  if (bt.B <= 0) DTC_TRY(auto_batch(ctx, per_state, reusable, large_state_rule, bt.B));
  if (max_B > 0) bt.B = std::max<int64_t>(1, std::min<int64_t>(bt.B, max_B));
  batch_layout(ctx, rc.pl.L_eff, bt.S, bt.B, bt.octet);
  if (prefix_octet >= 0) {
    bt.octet = prefix_octet;
    if (bt.octet && bt.B < bt.S) {
      bt.B &= ~(int64_t)7;
      if (bt.B < 8) return fail(DTC_EINVAL, "batch too small for the prefix's octet layout");
    }
  }
  rc.octet_bits = bt.octet;
  bt.Bp = dtc::octet_padded(bt.B, bt.octet);
  DTC_TRY(ensure(ctx->F, (size_t)(bt.Bp * rc.pl.len * 16)));
  if (need_E) DTC_TRY(ensure(ctx->E, (size_t)(bt.Bp * rc.pl.len * 16)));
  DTC_TRY(ensure(ctx->basis, (size_t)bt.B * sizeof(int64_t)));
  return DTC_OK;
}

// The initial basis states of batch [bs, bs + nb): their masks, and the upload
// to ctx->basis.
int batch_masks(dtc_ctx* ctx, const RunCfg& rc, int64_t bs, int nb, std::vector<int64_t>& masks) {
  for (int b = 0; b < nb; ++b)
    masks[b] = (int64_t)init_state_mask(rc, (uint64_t)(rc.traj_offset + (bs + b) % rc.n_traj));
  DTC_HIP(hipMemcpyAsync(ctx->basis.p, masks.data(), nb * sizeof(int64_t), hipMemcpyHostToDevice,
                         ctx->stream));
  return DTC_OK;
}

// What a prefixed run needs of the prefix in place (dtc_prefix_build).
int check_prefix(const dtc_ctx* ctx, const dtc_problem* pr, const RunCfg& rc, int64_t S,
                 bool device) {
  const int n_pre = ctx->prefix_periods;
  if (n_pre < 0) return fail(DTC_EINVAL, "no prefix built");
  if (ctx->prefix_states != S || ctx->prefix_n_traj != rc.n_traj ||
      ctx->prefix_traj_offset != rc.traj_offset || ctx->prefix_len != rc.pl.len ||
      ctx->prefix_device != (device ? 1 : 0))
    return fail(DTC_EINVAL, "prefix built for other trajectories / size / noise kind");
  if (pr->t_first + pr->t_offset <= n_pre || pr->T - 1 + pr->t_offset <= n_pre)
    return fail(DTC_EINVAL, "prefixed run must measure only after the prefix's periods");
  if (prefix_hash(pr, n_pre) != ctx->prefix_hash)
    return fail(DTC_EINVAL, "problem differs from the prefix's in angles or kick rows");
  return DTC_OK;
}

// A batch's finished autocorrelator rows -- hv_f[nb][T][n_obs_f] (the probe, or
// per-site Z when zsite) and hv_e[nb][T][2] -- into the caller's arrays (each
// nullable: not wanted).  fac: the ancilla gates' factor; read-out:
// measured = ro_a * a + ro_b (identity without device noise).
struct ReadOut {
  double fac, ro_a, ro_b;
};
void autocorr_rows_out(const RunCfg& rc, const ReadOut& ro, const double* hv_f, const double* hv_e,
                       const int64_t* masks, int64_t bs, int nb, double* fwd, double* echo,
                       double* zsite) {
  const dtc_problem* pr = rc.prob;
  const int T = pr->T, L = pr->L, j = pr->probe_site;
  const bool want_z = zsite != nullptr;
  const int n_obs_f = want_z ? 1 + L : 2;
  for (int b = 0; b < nb; ++b) {
    const int64_t g = bs + b;
    const uint64_t m = (uint64_t)masks[b];
    const double zinit = ((m >> j) & 1ull) ? -1.0 : 1.0;
    for (int t = std::max(0, pr->t_first); t < T; ++t) {
      const bool at_init = (t + pr->t_offset == 0);
      const double* vf = hv_f + ((size_t)b * T + t) * n_obs_f;
      // bond noise: the forward state at t is measured before its layer's
      // outgoing Pauli P_t, whose X content flips the sign of <Z_i>
      const uint64_t px =
          (rc.bond && !at_init)
              ? bond_out_x(rc, (uint64_t)(rc.traj_offset + g % rc.n_traj), dtc::kStreamForward,
                           (uint32_t)(t + pr->t_offset))
              : 0ull;
      const double zj_f = (at_init ? zinit : (want_z ? vf[1 + j] : vf[1])) *
                          (((px >> j) & 1ull) ? -1.0 : 1.0);
      if (fwd) fwd[(size_t)g * T + t] = ro.ro_a * (ro.fac * zinit * zj_f) + ro.ro_b;
      if (want_z) {
        double* zo = zsite + ((size_t)g * T + t) * L;
        for (int i = 0; i < L; ++i)
          zo[i] = at_init ? (((m >> i) & 1ull) ? -1.0 : 1.0)
                          : (((px >> i) & 1ull) ? -vf[1 + i] : vf[1 + i]);
      }
      if (echo) {
        const double zj_e = at_init ? zinit : hv_e[((size_t)b * T + t) * 2 + 1];
        echo[(size_t)g * T + t] = ro.ro_a * (ro.fac * zinit * zj_e) + ro.ro_b;
      }
    }
  }
}

// The new wavefront table sets of a schedule (the first batch's), uploaded
// while the stream is idle.
int upload_wf_tables(dtc_ctx* ctx, WfTables& wt) {
  if (!wt.dirty) return DTC_OK;
  DTC_HIP(hipStreamSynchronize(ctx->stream));
  DTC_TRY(ensure(ctx->wf_tab, wt.host.size() * sizeof(double)));
  DTC_HIP(hipMemcpy(ctx->wf_tab.p, wt.host.data(), wt.host.size() * sizeof(double),
                    hipMemcpyHostToDevice));
  wt.dirty = false;
  return DTC_OK;
}

// The energy echo's finished batch (vals_e[nb][T][3 L]) into the caller's arrays
// through the staging hv_e: the rows, or their per-instance sums
// (traj_sum_kernel into vals_f, as dtc_energy_sums).
int energy_echo_out(dtc_ctx* ctx, const dtc_problem* pr, const EchoEnergyOut& ee,
                    const int64_t* masks, int64_t bs, int nb, int n_traj, double* hv_e) {
  const size_t vs = (size_t)pr->T * 3 * pr->L;
  size_t n_rows = (size_t)nb;
  const double* rows = (const double*)ctx->vals_e.p;
  if (ee.sums) {
    n_rows = (size_t)((bs + nb - 1) / n_traj - bs / n_traj + 1);
    DTC_HIP(dtc::launch_traj_sum(rows, nb, (int)vs, bs, n_traj, (double*)ctx->vals_f.p,
                                 ctx->stream));
    rows = (const double*)ctx->vals_f.p;
  }
  DTC_HIP(hipMemcpyAsync(hv_e, rows, n_rows * vs * sizeof(double), hipMemcpyDeviceToHost,
                         ctx->stream));
  DTC_HIP(hipStreamSynchronize(ctx->stream));
  DTC_TRY(settle_pending(ctx));
  if (ee.sums)
    energy_sums_out(pr, hv_e, masks, bs, nb, n_traj, pr->t_first, ee.z, ee.zz, ee.x);
  else
    energy_rows_out(pr, hv_e, masks, bs, nb, pr->t_first, ee.z, ee.zz, ee.x);
  return DTC_OK;
}

int autocorr_impl(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz,
                  const dtc_device_noise* dv, uint64_t seed, int64_t traj_offset, int32_t n_traj,
                  double* fwd, double* echo, double* zsite, bool use_prefix = false,
                  const dtc_bond_noise* bond = nullptr, const EchoEnergyOut* ee = nullptr) {
  if (!ctx) return fail(DTC_EINVAL, "null ctx");
  DTC_TRY(check_problem(pr, nz));
  RunCfg rc;
  DTC_TRY(init_run_cfg(ctx, pr, nz, dv, bond, seed, traj_offset, n_traj,
                       !dv && !zsite && !use_prefix && !bond && !ee, rc));
  // (the energy echo ignores want_fwd / want_echo: the echo chains only)
  const bool want_fwd = !ee && pr->want_fwd, want_echo = ee || pr->want_echo;
  if (want_fwd && !fwd) return fail(DTC_EINVAL, "want_fwd but fwd is null");
  if (!ee && want_echo && !echo) return fail(DTC_EINVAL, "want_echo but echo is null");
  if (ee && (dv || bond || zsite || use_prefix))
    return fail(DTC_EINVAL, "internal: the energy echo runs depolarizing or noiseless chains only");
  const Plan& pl = rc.pl;
  const int T = pr->T, L = pr->L;
  const bool want_z = zsite != nullptr;
  const bool want_e = want_echo;
  // energy echo: a chain's row is norm, Z_i | Z_i Z_i+1 | X_i (energy_impl's)
  const int n_v = 3 * L;
  const int n_obs_f = want_z ? 1 + L : 2, n_obs_e = ee ? n_v : 2;
  const ReadOut ro{dv ? dv->anc_factor : std::pow(1.0 - nz->p, (double)nz->n_anc),
                   dv ? 1.0 - dv->readout_p01 - dv->readout_p10 : 1.0,
                   dv ? dv->readout_p10 - dv->readout_p01 : 0.0};

  DTC_TRY(upload_tables(ctx, pr, pl));

  // batch size: F (+ E for echo) resident in HBM
  const int64_t S = (int64_t)pr->n_inst * n_traj;
  // continuation of a prefix: periods 1..n_pre come from dtc_prefix_build
  if (use_prefix) DTC_TRY(check_prefix(ctx, pr, rc, S, dv != nullptr));
  const double per_state = (double)pl.len * 16.0 * (want_e ? 2.0 : 1.0);
  // (the prefix's states are in the layout they were built in)
  Batch bt;
  DTC_TRY(plan_batch(ctx, rc, per_state, ctx->F.n + ctx->E.n, true, 0, want_e,
                     use_prefix ? ctx->prefix_octet : -1, bt));
  const int64_t B = bt.B;
  const int octet = bt.octet;
  if (ctx->verbose) {
    size_t fr = 0, to = 0;
    (void)hipMemGetInfo(&fr, &to);
    std::fprintf(stderr, "[dtc] L=%d states=%lld batch=%lld state=%.3f GiB free=%.1f/%.1f GiB\n",
                 L, (long long)S, (long long)B, per_state / (1 << 30), fr / 1073741824.0,
                 to / 1073741824.0);
  }

  const int max_obs = std::max(n_obs_f, n_obs_e);
  DTC_TRY(ensure(ctx->partial, (size_t)B * pl.n_tiles * max_obs * sizeof(double)));
  DTC_TRY(ensure(ctx->vals_f, (size_t)B * T * n_obs_f * sizeof(double)));
  if (want_e) DTC_TRY(ensure(ctx->vals_e, (size_t)B * T * n_obs_e * sizeof(double)));
  // energy echo sums: at most (B - 1) / n_traj + 2 instances per batch, summed
  // on the device into vals_f (the forward is not measured)
  const int64_t max_inst_b = std::min<int64_t>(pr->n_inst, (B - 1) / n_traj + 2);
  if (ee && ee->sums) {
    DTC_TRY(ensure(ctx->vals_f, (size_t)max_inst_b * T * n_v * sizeof(double)));
    const size_t n_out = (size_t)pr->n_inst * T;
    std::fill(ee->z, ee->z + n_out * L, 0.0);
    std::fill(ee->x, ee->x + n_out * L, 0.0);
    if (L > 1) std::fill(ee->zz, ee->zz + n_out * (L - 1), 0.0);
  }
  if (rc.bond) DTC_TRY(ensure(ctx->bond_diag, (size_t)B * pl.diag_stride * sizeof(double2)));

  DTC_TRY(ensure_host(ctx->host_f, (size_t)B * T * n_obs_f));
  if (want_e)
    DTC_TRY(ensure_host(ctx->host_e, (size_t)((ee && ee->sums) ? max_inst_b : B) * T * n_obs_e));
  double* const hv_f = ctx->host_f.p;
  double* const hv_e = ctx->host_e.p;
  std::vector<int64_t> masks(B);
  const SchedReq rq{want_fwd, want_echo, want_z ? dtc::kMeasSites : dtc::kMeasProbe, n_obs_f,
                    ee != nullptr, use_prefix ? ctx->prefix_periods : 0, octet};
  WfTables wf_tables;
  std::vector<Launch> sched;

  for (int64_t bs = 0; bs < S; bs += B) {
    const int nb = (int)std::min<int64_t>(B, S - bs);
    if (use_prefix)
      std::copy_n(ctx->prefix_masks.begin() + bs, nb, masks.begin());
    else
      DTC_TRY(batch_masks(ctx, rc, bs, nb, masks));
    double2* F = (double2*)ctx->F.p;
    double2* E = (double2*)ctx->E.p;
#ifdef DTC_DEV_KNOBS
    // development builds: DTC_FE_SWAP=1 runs the forward in the echo buffer and
    // the echo chains in the forward buffer (buffer-placement A/B)
    if (want_e && !use_prefix && std::getenv("DTC_FE_SWAP")) std::swap(F, E);
#endif
    // the first forward pass reads the prefix states (or the basis states in F)
    // (bs is a multiple of 8 in the octet layout: the batch starts an octet)
    const double2* F0 = use_prefix ? (const double2*)ctx->prefix.p + (size_t)bs * pl.len : F;
    DTC_HIP(hipMemsetAsync(ctx->vals_f.p, 0, (size_t)nb * T * n_obs_f * sizeof(double),
                           ctx->stream));
    if (want_e)
      DTC_HIP(hipMemsetAsync(ctx->vals_e.p, 0, (size_t)nb * T * n_obs_e * sizeof(double),
                             ctx->stream));

    // the whole batch schedule is built first (dtc_schedule.h), once per batch
    const SchedBufs bufs{F0, F, E, (double*)ctx->vals_f.p, (double*)ctx->vals_e.p};
    SchedInfo info;
    if (const char* err = build_autocorr_schedule(rc, ctx->so, rq, bufs, wf_tables, sched, info))
      return fail(DTC_EINVAL, err);
    if (info.rebuilt && ctx->verbose)
      std::fprintf(stderr, "[dtc] device-noise schedule rebuilt with K-D forward passes "
                           "(an echo chain did not fold into the dual pass)\n");
    ctx->sched_counts[0] += info.n_folds;
    if (rc.device) ++ctx->sched_counts[info.dev_ahead ? 1 : 2];
    if (pl.groups[0].tb == dtc::kMaxTileBits) ++ctx->sched_counts[3];
    DTC_TRY(upload_wf_tables(ctx, wf_tables));
    if (!use_prefix) DTC_TRY(basis_source(ctx, sched, F, pl.len, nb, octet));
    DTC_TRY(run_launches(ctx, rc, bs, nb, sched));
    if (ee) {
      DTC_TRY(energy_echo_out(ctx, pr, *ee, masks.data(), bs, nb, n_traj, hv_e));
      continue;
    }
    DTC_HIP(hipMemcpyAsync(hv_f, ctx->vals_f.p, (size_t)nb * T * n_obs_f * sizeof(double),
                           hipMemcpyDeviceToHost, ctx->stream));
    if (want_e)
      DTC_HIP(hipMemcpyAsync(hv_e, ctx->vals_e.p, (size_t)nb * T * 2 * sizeof(double),
                             hipMemcpyDeviceToHost, ctx->stream));
    DTC_HIP(hipStreamSynchronize(ctx->stream));
    DTC_TRY(settle_pending(ctx));
    autocorr_rows_out(rc, ro, hv_f, hv_e, masks.data(), bs, nb, want_fwd ? fwd : nullptr,
                      want_e ? echo : nullptr, zsite);
  }
  return DTC_OK;
}

// Forward prefix: the initial states of all n_inst * n_traj trajectories
// taken through periods 1..n_periods (post_after_d as the forward chain of
// autocorr_impl, so no kick is pending) into ctx->prefix, in batches in place.
int prefix_build_impl(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz,
                      const dtc_device_noise* dv, uint64_t seed, int64_t traj_offset,
                      int32_t n_traj, int32_t n_periods) {
  if (!ctx) return fail(DTC_EINVAL, "null ctx");
  DTC_TRY(check_problem(pr, nz));
  RunCfg rc;
  DTC_TRY(init_run_cfg(ctx, pr, nz, dv, nullptr, seed, traj_offset, n_traj, false, rc));
  if (n_periods < 1 || n_periods > pr->T - 1 + pr->t_offset)
    return fail(DTC_EINVAL, "n_periods must be in [1, T - 1 + t_offset]");
  const Plan& pl = rc.pl;
  DTC_TRY(upload_tables(ctx, pr, pl));
  const int64_t S = (int64_t)pr->n_inst * n_traj;
  ctx->prefix_periods = -1;
  // batches of up to 4096 states (multiples of 8): the octet layout whenever
  // there is an octet; autocorr_prefixed reads them in this layout
  int64_t B = 4096;
  int octet = 0;
  batch_layout(ctx, pl.L_eff, S, B, octet);
  rc.octet_bits = octet;
  DTC_TRY(ensure(ctx->prefix, (size_t)dtc::octet_padded(S, octet) * pl.len * 16));
  ctx->prefix_masks.resize(S);
  for (int64_t g = 0; g < S; ++g)
    ctx->prefix_masks[g] = (int64_t)init_state_mask(rc, (uint64_t)(traj_offset + g % n_traj));
  DTC_TRY(ensure(ctx->basis, (size_t)B * sizeof(int64_t)));
  for (int64_t bs = 0; bs < S; bs += B) {
    const int nb = (int)std::min<int64_t>(B, S - bs);
    double2* F = (double2*)ctx->prefix.p + (size_t)bs * pl.len;
    DTC_HIP(hipMemcpyAsync(ctx->basis.p, ctx->prefix_masks.data() + bs, nb * sizeof(int64_t),
                           hipMemcpyHostToDevice, ctx->stream));
    std::vector<Launch> sched = build_prefix_schedule(rc, n_periods, F);
    DTC_TRY(basis_source(ctx, sched, F, pl.len, nb, octet));
    DTC_TRY(run_launches(ctx, rc, bs, nb, sched));
    DTC_HIP(hipStreamSynchronize(ctx->stream));  // the staged pass list is reused
  }
  DTC_TRY(settle_pending(ctx));
  ctx->prefix_periods = n_periods;
  ctx->prefix_states = S;
  ctx->prefix_traj_offset = traj_offset;
  ctx->prefix_n_traj = n_traj;
  ctx->prefix_len = pl.len;
  ctx->prefix_device = dv ? 1 : 0;
  ctx->prefix_octet = octet;
  ctx->prefix_hash = prefix_hash(pr, n_periods);
  return DTC_OK;
}

}  // namespace

extern "C" {

int dtc_autocorr(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz, uint64_t seed,
                 int64_t traj_offset, int32_t n_traj, double* fwd, double* echo,
                 double* zsite) {
  return autocorr_impl(ctx, pr, nz, nullptr, seed, traj_offset, n_traj, fwd, echo, zsite);
}

int dtc_autocorr_device(dtc_ctx* ctx, const dtc_problem* pr, const dtc_device_noise* dv,
                        uint64_t seed, int64_t traj_offset, int32_t n_traj, double* fwd,
                        double* echo, double* zsite) {
  if (!dv) return fail(DTC_EINVAL, "null device noise");
  const dtc_noise nz{0.0, 0, 0};
  return autocorr_impl(ctx, pr, &nz, dv, seed, traj_offset, n_traj, fwd, echo, zsite);
}

int dtc_autocorr_bond(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz,
                      const dtc_device_noise* dv, const dtc_bond_noise* bond, uint64_t seed,
                      int64_t traj_offset, int32_t n_traj, double* fwd, double* echo,
                      double* zsite) {
  // device-like noise: `noise` is ignored, as in dtc_autocorr_device
  const dtc_noise none{0.0, 0, 0};
  if (dv) nz = &none;
  DTC_TRY(check_problem(pr, nz));
  std::vector<uint32_t> thr;
  DTC_TRY(bond_thresholds(bond, pr->L, thr));
  if (!ctx) return fail(DTC_EINVAL, "null ctx");
  bool any = false;
  for (uint32_t v : thr) any = any || v != 0u;
  // no bond, or no bond can err: exactly dtc_autocorr / dtc_autocorr_device
  if (!any) return autocorr_impl(ctx, pr, nz, dv, seed, traj_offset, n_traj, fwd, echo, zsite);
  if (pr->t_offset != 0) return fail(DTC_EINVAL, "bond noise needs t_offset = 0");
  if (ctx->prefix_periods >= 0)
    return fail(DTC_EINVAL, "bond noise cannot run with a forward prefix in place "
                            "(dtc_prefix_release first)");
  return autocorr_impl(ctx, pr, nz, dv, seed, traj_offset, n_traj, fwd, echo, zsite, false, bond);
}

int dtc_kick_draws(const dtc_noise* nz, const dtc_device_noise* dv, int32_t L, int32_t n_sub,
                   uint64_t seed, int64_t traj, uint32_t stream, uint32_t counter, int32_t* pauli,
                   int32_t* jump) {
  if ((!nz && !dv) || !pauli) return fail(DTC_EINVAL, "null noise/pauli");
  if (L < 1 || L > 32) return fail(DTC_EINVAL, "L must be in [1, 32]");
  if (n_sub < 1 || n_sub > 8) return fail(DTC_EINVAL, "n_sub must be in [1, 8]");
  if (traj < 0) return fail(DTC_EINVAL, "traj must be >= 0");
  if (dv) {
    std::vector<uint32_t> thr, thr_jump;
    std::vector<double> kraus;
    DTC_TRY(device_noise_tables(dv, L, thr, thr_jump, kraus));
    // the neel preparation draws its Pauli only (init_state_mask)
    const bool prep = stream == dtc::kStreamPrep;
    for (int i = 0; i < L; ++i)
      for (int q = 0; q < n_sub; ++q) {
        int j = 0;
        pauli[i * n_sub + q] =
            dtc::sample_device(seed, (uint64_t)traj, stream, counter, (uint32_t)i, (uint32_t)q,
                               thr.data() + 3 * i, prep ? 0u : thr_jump[i], &j);
        if (jump) jump[i * n_sub + q] = j;
      }
    return DTC_OK;
  }
  if (!(nz->p >= 0.0) || nz->p > 4.0 / 3.0) return fail(DTC_EINVAL, "noise p out of range");
  uint32_t t1, t2, t3;
  thresholds(nz->p, &t1, &t2, &t3);
  for (int i = 0; i < L; ++i)
    for (int q = 0; q < n_sub; ++q) {
      pauli[i * n_sub + q] = nz->p > 0.0 ? dtc::sample_pauli(seed, (uint64_t)traj, stream, counter,
                                                             (uint32_t)i, (uint32_t)q, t1, t2, t3)
                                         : 0;
      if (jump) jump[i * n_sub + q] = 0;
    }
  return DTC_OK;
}

int dtc_bond_draws(const dtc_bond_noise* bond, int32_t L, uint64_t seed, int64_t traj,
                   uint32_t stream, uint32_t counter, int32_t* codes) {
  if (!bond || !codes) return fail(DTC_EINVAL, "null bond/codes");
  if (L < 1 || L > 32) return fail(DTC_EINVAL, "L must be in [1, 32]");
  if (traj < 0) return fail(DTC_EINVAL, "traj must be >= 0");
  std::vector<uint32_t> thr;
  DTC_TRY(bond_thresholds(bond, L, thr));
  for (int b = 0; b + 1 < L; ++b)
    codes[b] = dtc::sample_bond(seed, (uint64_t)traj, stream, counter, (uint32_t)b, thr[b]);
  return DTC_OK;
}

int dtc_prefix_build(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz,
                     const dtc_device_noise* dv, uint64_t seed, int64_t traj_offset,
                     int32_t n_traj, int32_t n_periods) {
  const dtc_noise none{0.0, 0, 0};
  if (!dv && !nz) return fail(DTC_EINVAL, "null noise");
  return prefix_build_impl(ctx, pr, dv ? &none : nz, dv, seed, traj_offset, n_traj, n_periods);
}

int dtc_autocorr_prefixed(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz,
                          const dtc_device_noise* dv, uint64_t seed, int64_t traj_offset,
                          int32_t n_traj, double* fwd, double* echo) {
  const dtc_noise none{0.0, 0, 0};
  if (!dv && !nz) return fail(DTC_EINVAL, "null noise");
  return autocorr_impl(ctx, pr, dv ? &none : nz, dv, seed, traj_offset, n_traj, fwd, echo,
                       nullptr, true);
}

int dtc_prefix_release(dtc_ctx* ctx) {
  if (!ctx) return fail(DTC_EINVAL, "null ctx");
  DTC_HIP(hipStreamSynchronize(ctx->stream));
  release(ctx->prefix);
  ctx->prefix_masks.clear();
  ctx->prefix_periods = -1;
  return DTC_OK;
}

int dtc_apply_periods(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz, uint64_t seed,
                      int32_t inst, int64_t traj, uint32_t stream, int32_t first_period,
                      int32_t n_periods, int32_t inverse, double* state, double* zsite_out) {
  if (!ctx || !state) return fail(DTC_EINVAL, "null ctx/state");
  DTC_TRY(check_problem(pr, nz));
  if (inst < 0 || inst >= pr->n_inst) return fail(DTC_EINVAL, "inst out of range");
  if (traj < 0) return fail(DTC_EINVAL, "traj must be >= 0");
  if (n_periods < 0) return fail(DTC_EINVAL, "n_periods must be >= 0");
  const int n_rows = std::max(1, pr->T - 1 + pr->t_offset);
  if (n_periods > 0) {
    const int lo = inverse ? first_period - n_periods + 1 : first_period;
    const int hi = inverse ? first_period : first_period + n_periods - 1;
    if (lo < 1 || hi > n_rows) return fail(DTC_EINVAL, "period range outside kick table");
  }
  DTC_HIP(hipSetDevice(ctx->device));
  RunCfg rc;
  rc.prob = pr;
  rc.pl = make_plan(pr->L);
  rc.seed = seed;
  rc.traj_offset = traj;
  rc.n_traj = 1;
  rc.noisy = nz->p > 0.0 ? 1 : 0;
  rc.row_kind = classify_rows(pr);
  thresholds(nz->p, &rc.thr1, &rc.thr2, &rc.thr3);
  const Plan& pl = rc.pl;
  const int L = pr->L;
  DTC_TRY(upload_tables(ctx, pr, pl));
  DTC_TRY(ensure(ctx->F, (size_t)pl.len * 16));
  DTC_TRY(ensure(ctx->partial, (size_t)pl.n_tiles * (1 + L) * sizeof(double)));
  DTC_TRY(ensure(ctx->vals_f, (size_t)(1 + L) * sizeof(double)));
  double2* F = (double2*)ctx->F.p;
  DTC_HIP(hipMemsetAsync(F, 0, (size_t)pl.len * 16, ctx->stream));
  DTC_HIP(hipMemcpyAsync(F, state, ((size_t)1 << L) * 16, hipMemcpyHostToDevice, ctx->stream));
  const int64_t batch_start = inst;  // n_traj = 1: g = inst -> (inst, traj)
  if (n_periods > 0) {
    Chain ch;
    if (inverse) {
      ch = echo_chain(pl, first_period, stream, std::vector<int>(pl.groups.size(), 0));
      // echo_chain counts periods p..1; re-base so the first inverse period is
      // first_period and there are n_periods of them
      ch.X.resize(1);
      for (int k = 1; k <= n_periods; ++k)
        ch.X.push_back(dtc::KickDesc{1, first_period - k, dtc::kKickInverse, stream,
                                     (uint32_t)k});
    } else {
      ch = forward_chain(pl, first_period, n_periods, stream);
    }
    DTC_TRY(run_chain(ctx, rc, batch_start, 1, ch, F, F,
                      zsite_out ? dtc::kMeasSites : dtc::kMeasNone, 1 + L,
                      (double*)ctx->vals_f.p, 1 + L));
  }
  DTC_HIP(hipMemcpyAsync(state, F, ((size_t)1 << L) * 16, hipMemcpyDeviceToHost, ctx->stream));
  if (zsite_out && n_periods > 0)
    DTC_HIP(hipMemcpyAsync(zsite_out, ctx->vals_f.p, (size_t)(1 + L) * sizeof(double),
                           hipMemcpyDeviceToHost, ctx->stream));
  DTC_HIP(hipStreamSynchronize(ctx->stream));
  DTC_TRY(settle_pending(ctx));
  if (zsite_out && n_periods == 0) {
    // no kernel ran: reduce on the host copy
    std::vector<double> acc(1 + L, 0.0);
    for (size_t x = 0; x < ((size_t)1 << L); ++x) {
      const double pr2 = state[2 * x] * state[2 * x] + state[2 * x + 1] * state[2 * x + 1];
      acc[0] += pr2;
      for (int i = 0; i < L; ++i) acc[1 + i] += ((x >> i) & 1) ? -pr2 : pr2;
    }
    for (int i = 0; i <= L; ++i) zsite_out[i] = acc[i];
  }
  return DTC_OK;
}

namespace {

// sums: z, zz, x are per-instance sums over the trajectories ([n_inst][T][.],
// dtc_energy_sums) instead of per-trajectory rows
int energy_impl(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz,
                const dtc_device_noise* dv, uint64_t seed, int64_t traj_offset, int32_t n_traj,
                double* z, double* zz, double* x, bool sums = false,
                const dtc_bond_noise* bond = nullptr) {
  if (!ctx || !z || !x || (!zz && pr && pr->L > 1)) return fail(DTC_EINVAL, "null ctx/outputs");
  DTC_TRY(check_problem(pr, nz));
  RunCfg rc;
  DTC_TRY(init_run_cfg(ctx, pr, nz, dv, bond, seed, traj_offset, n_traj, false, rc));
  const Plan& pl = rc.pl;
  const int T = pr->T, L = pr->L;
  const int n_v = 3 * L;    // per time: norm, Z_i, Z_i Z_i+1, X_i
  const int n_obs = 4 * L;  // per pass: the above (mid-pass) + X_i before the pre-kick
  if (n_obs > dtc::kThreads) return fail(DTC_EINVAL, "dtc_energy: L > 64");
  DTC_TRY(upload_tables(ctx, pr, pl));

  // (device-like noise: E too, for the X-basis passes)
  const double per_state = (double)pl.len * 16.0 * (dv ? 2.0 : 1.0);
  Batch bt;
  DTC_TRY(plan_batch(ctx, rc, per_state, ctx->F.n + (dv ? ctx->E.n : 0), false, 0, dv != nullptr,
                     -1, bt));
  const int64_t S = bt.S, B = bt.B;
  DTC_TRY(ensure(ctx->partial, (size_t)B * pl.n_tiles * n_obs * sizeof(double)));
  DTC_TRY(ensure(ctx->vals_f, (size_t)B * T * n_v * sizeof(double)));
  if (rc.bond) DTC_TRY(ensure(ctx->bond_diag, (size_t)B * pl.diag_stride * sizeof(double2)));
  // per-instance sums: at most (B - 1) / n_traj + 2 instances per batch
  const int64_t max_inst_b = std::min<int64_t>(pr->n_inst, (B - 1) / n_traj + 2);
  if (sums) {
    DTC_TRY(ensure(ctx->vals_e, (size_t)max_inst_b * T * n_v * sizeof(double)));
    const size_t n_out = (size_t)pr->n_inst * T;
    std::fill(z, z + n_out * L, 0.0);
    std::fill(x, x + n_out * L, 0.0);
    if (L > 1) std::fill(zz, zz + n_out * (L - 1), 0.0);
  }
  DTC_TRY(ensure_host(ctx->host_f, (size_t)(sums ? max_inst_b : B) * T * n_v));
  double* const hv_f = ctx->host_f.p;
  std::vector<int64_t> masks(B);

  // the schedule (build_energy_schedule, dtc_schedule.h) is the same for every
  // batch; under device-like noise the pass that leaves the state at a time is
  // followed by that state's X: E = H^L F, per-site Z of E into the row's X part
  double2* const F = (double2*)ctx->F.p;
  double* const vals = (double*)ctx->vals_f.p;
  std::vector<Launch> sched;
  if (const char* err = build_energy_schedule(rc, F, vals, sched)) return fail(DTC_EINVAL, err);
  const int64_t vs = (int64_t)T * n_v;

  for (int64_t bs = 0; bs < S; bs += B) {
    const int nb = (int)std::min<int64_t>(B, S - bs);
    DTC_TRY(batch_masks(ctx, rc, bs, nb, masks));
    DTC_TRY(basis_source(ctx, sched, F, pl.len, nb, bt.octet));
    DTC_HIP(hipMemsetAsync(vals, 0, (size_t)nb * T * n_v * sizeof(double), ctx->stream));
    const AfterLaunch x_row = [&](const Launch& l) -> int {
      DTC_TRY(launch_xbasis(ctx, rc, bs, nb, F, (double2*)ctx->E.p, true));
      return launch_reduce_prof(ctx, pl.n_tiles, 1 + L, nb, l.energy_row + 2 * L, vs, 1, L, 1);
    };
    DTC_TRY(run_launches(ctx, rc, bs, nb, sched, x_row));
    if (rc.bond) DTC_TRY(launch_bond_signs(ctx, rc, bs, nb, vals, T));
    if (sums) {
      // the batch's rows summed per instance on the device (the rows of the
      // initial time are formed from the masks below, not read)
      const int64_t i0 = bs / n_traj, n_ib = (bs + nb - 1) / n_traj - i0 + 1;
      DTC_HIP(dtc::launch_traj_sum(vals, nb, (int)vs, bs, n_traj, (double*)ctx->vals_e.p,
                                   ctx->stream));
      DTC_HIP(hipMemcpyAsync(hv_f, ctx->vals_e.p, (size_t)n_ib * vs * sizeof(double),
                             hipMemcpyDeviceToHost, ctx->stream));
      DTC_HIP(hipStreamSynchronize(ctx->stream));
      DTC_TRY(settle_pending(ctx));
      energy_sums_out(pr, hv_f, masks.data(), bs, nb, n_traj, 0, z, zz, x);
      continue;
    }
    DTC_HIP(hipMemcpyAsync(hv_f, vals, (size_t)nb * T * n_v * sizeof(double),
                           hipMemcpyDeviceToHost, ctx->stream));
    DTC_HIP(hipStreamSynchronize(ctx->stream));
    DTC_TRY(settle_pending(ctx));
    energy_rows_out(pr, hv_f, masks.data(), bs, nb, 0, z, zz, x);
  }
  return DTC_OK;
}

}  // namespace

int dtc_energy(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz, uint64_t seed,
               int64_t traj_offset, int32_t n_traj, double* z, double* zz, double* x) {
  return energy_impl(ctx, pr, nz, nullptr, seed, traj_offset, n_traj, z, zz, x);
}

int dtc_energy_device(dtc_ctx* ctx, const dtc_problem* pr, const dtc_device_noise* dv,
                      uint64_t seed, int64_t traj_offset, int32_t n_traj, double* z, double* zz,
                      double* x) {
  if (!dv) return fail(DTC_EINVAL, "null device noise");
  const dtc_noise nz{0.0, 0, 0};
  return energy_impl(ctx, pr, &nz, dv, seed, traj_offset, n_traj, z, zz, x);
}

int dtc_energy_sums(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz,
                    const dtc_device_noise* dv, uint64_t seed, int64_t traj_offset,
                    int32_t n_traj, double* z_sum, double* zz_sum, double* x_sum) {
  if (dv) {
    const dtc_noise none{0.0, 0, 0};
    return energy_impl(ctx, pr, &none, dv, seed, traj_offset, n_traj, z_sum, zz_sum, x_sum, true);
  }
  if (!nz) return fail(DTC_EINVAL, "null noise");
  return energy_impl(ctx, pr, nz, nullptr, seed, traj_offset, n_traj, z_sum, zz_sum, x_sum, true);
}

int dtc_energy_echo(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz, uint64_t seed,
                    int64_t traj_offset, int32_t n_traj, double* z, double* zz, double* x) {
  if (!ctx || !z || !x || (!zz && pr && pr->L > 1)) return fail(DTC_EINVAL, "null ctx/outputs");
  const EchoEnergyOut ee{z, zz, x, false};
  return autocorr_impl(ctx, pr, nz, nullptr, seed, traj_offset, n_traj, nullptr, nullptr, nullptr,
                       false, nullptr, &ee);
}

int dtc_energy_echo_sums(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz, uint64_t seed,
                         int64_t traj_offset, int32_t n_traj, double* z_sum, double* zz_sum,
                         double* x_sum) {
  if (!ctx || !z_sum || !x_sum || (!zz_sum && pr && pr->L > 1))
    return fail(DTC_EINVAL, "null ctx/outputs");
  const EchoEnergyOut ee{z_sum, zz_sum, x_sum, true};
  return autocorr_impl(ctx, pr, nz, nullptr, seed, traj_offset, n_traj, nullptr, nullptr, nullptr,
                       false, nullptr, &ee);
}

namespace {

// The energy entry points with bond noise: dv nullable (then `noise` is used).
int energy_bond_impl(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz,
                     const dtc_device_noise* dv, const dtc_bond_noise* bond, uint64_t seed,
                     int64_t traj_offset, int32_t n_traj, double* z, double* zz, double* x,
                     bool sums) {
  const dtc_noise none{0.0, 0, 0};
  if (dv) nz = &none;
  DTC_TRY(check_problem(pr, nz));
  std::vector<uint32_t> thr;
  DTC_TRY(bond_thresholds(bond, pr->L, thr));
  bool any = false;
  for (uint32_t v : thr) any = any || v != 0u;
  // no bond, or no bond can err: exactly the plain entry points
  return energy_impl(ctx, pr, nz, dv, seed, traj_offset, n_traj, z, zz, x, sums,
                     any ? bond : nullptr);
}

}  // namespace

int dtc_energy_bond(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz,
                    const dtc_device_noise* dv, const dtc_bond_noise* bond, uint64_t seed,
                    int64_t traj_offset, int32_t n_traj, double* z, double* zz, double* x) {
  return energy_bond_impl(ctx, pr, nz, dv, bond, seed, traj_offset, n_traj, z, zz, x, false);
}

int dtc_energy_sums_bond(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz,
                         const dtc_device_noise* dv, const dtc_bond_noise* bond, uint64_t seed,
                         int64_t traj_offset, int32_t n_traj, double* z_sum, double* zz_sum,
                         double* x_sum) {
  return energy_bond_impl(ctx, pr, nz, dv, bond, seed, traj_offset, n_traj, z_sum, zz_sum, x_sum,
                          true);
}

namespace {

// The two sampling launches on a batch's states `st` (F, or E = H^L F) for time
// row t: weights, then one pick per (state, shot) into out[b][t][.].  Booked
// under DTC_KERNEL_REDUCE: the weights with the batch's 16 B per amplitude, the
// pick with the chunk weights and the one chunk each workgroup reads.
int launch_sample(dtc_ctx* ctx, const RunCfg& rc, int64_t batch_start, int batch,
                  const double2* st, int t, uint32_t basis, int n_shots, uint64_t* out) {
  dtc::SampleArgs A{};
  A.state = st;
  A.weights = (double*)ctx->sample_w.p;
  A.out = out + (size_t)t * n_shots;
  A.out_stride = (int64_t)rc.prob->T * n_shots;
  A.L_eff = rc.pl.L_eff;
  A.octet_bits = rc.octet_bits;
  A.batch = batch;
  A.n_shots = n_shots;
  A.batch_start = batch_start;
  A.n_traj = rc.n_traj;
  A.traj_offset = rc.traj_offset;
  A.seed = rc.seed;
  A.period = (uint32_t)(t + rc.prob->t_offset);
  A.basis = basis;
  DTC_TIMED(ctx, DTC_KERNEL_REDUCE, 16.0 * (double)rc.pl.len * batch,
            dtc::launch_sample_weights(A, ctx->stream));
  DTC_TIMED(ctx, DTC_KERNEL_REDUCE,
            (double)batch * n_shots * (8.0 * rc.pl.n_tiles + 16.0 * dtc::kTile),
            dtc::launch_sample_pick(A, ctx->stream));
  return DTC_OK;
}

}  // namespace

int dtc_sample(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz, uint64_t seed,
               int64_t traj_offset, int32_t n_traj, int32_t n_shots, uint64_t* zbits,
               uint64_t* xbits) {
  if (!ctx || (!zbits && !xbits)) return fail(DTC_EINVAL, "null ctx/outputs");
  if (n_shots < 1 || n_shots > (1 << 30))
    return fail(DTC_EINVAL, "n_shots must be in [1, 2^30]");
  DTC_TRY(check_problem(pr, nz));
  RunCfg rc;
  DTC_TRY(init_run_cfg(ctx, pr, nz, nullptr, nullptr, seed, traj_offset, n_traj, false, rc));
  const Plan& pl = rc.pl;
  const int T = pr->T, L = pr->L;
  const int P = T - 1 + pr->t_offset;
  const int64_t S = (int64_t)pr->n_inst * n_traj;
  const size_t row = (size_t)T * n_shots;  // outcomes per state and basis
  if (zbits) std::fill(zbits, zbits + (size_t)S * row, (uint64_t)0);
  if (xbits) std::fill(xbits, xbits + (size_t)S * row, (uint64_t)0);

  // Row p = 0: the rule on the prepared basis state |m>.  Z: every outcome is
  // m.  X: H^L |m> has weight 2^-L on every index, S(x) = (x + 1) 2^-L, so the
  // outcome is floor(u 2^L) (exact: u is a multiple of 2^-53, L <= 32).
  if (pr->t_offset == 0 && pr->t_first == 0) {
    for (int64_t s = 0; s < S; ++s) {
      const uint64_t traj = (uint64_t)(traj_offset + s % n_traj);
      const uint64_t m = init_state_mask(rc, traj);
      for (int k = 0; k < n_shots; ++k) {
        if (zbits) zbits[(size_t)s * row + k] = m;
        if (xbits)
          xbits[(size_t)s * row + k] =
              (uint64_t)std::floor(std::ldexp(dtc::sample_uniform(seed, traj, 0u, 1u, (uint32_t)k), L));
      }
    }
  }
  if (P == 0) return DTC_OK;
  DTC_TRY(upload_tables(ctx, pr, pl));

  // (the outcomes of a batch: at most 1 GiB)
  const double per_state = (double)pl.len * 16.0 * (xbits ? 2.0 : 1.0);
  Batch bt;
  DTC_TRY(plan_batch(ctx, rc, per_state, ctx->F.n + (xbits ? ctx->E.n : 0), false,
                     std::max<int64_t>(1, (int64_t)((size_t)(1u << 27) / row / 2)), xbits != nullptr,
                     -1, bt));
  const int64_t B = bt.B;
  DTC_TRY(ensure(ctx->sample_w, (size_t)B * pl.n_tiles * sizeof(double)));
  DTC_TRY(ensure(ctx->sample_bits, 2 * (size_t)B * row * sizeof(uint64_t)));
  std::vector<int64_t> masks(B);

  // the schedule (build_sample_schedule, dtc_schedule.h) is the same for every
  // batch; the state a pass leaves at a time is sampled in Z from F, in X from
  // E = H^L F
  double2* const F = (double2*)ctx->F.p;
  uint64_t* const zb = (uint64_t*)ctx->sample_bits.p;
  uint64_t* const xb = zb + (size_t)B * row;
  std::vector<Launch> sched = build_sample_schedule(rc, F);

  for (int64_t bs = 0; bs < S; bs += B) {
    const int nb = (int)std::min<int64_t>(B, S - bs);
    DTC_TRY(batch_masks(ctx, rc, bs, nb, masks));
    DTC_TRY(basis_source(ctx, sched, F, pl.len, nb, bt.octet));
    const AfterLaunch sample = [&](const Launch& l) -> int {
      if (zbits) DTC_TRY(launch_sample(ctx, rc, bs, nb, F, l.t_state, 0u, n_shots, zb));
      if (!xbits) return DTC_OK;
      double2* E = (double2*)ctx->E.p;
      DTC_TRY(launch_xbasis(ctx, rc, bs, nb, F, E, false));
      return launch_sample(ctx, rc, bs, nb, E, l.t_state, 1u, n_shots, xb);
    };
    DTC_TRY(run_launches(ctx, rc, bs, nb, sched, sample));
    // rows the device did not write (t < t_first, and p = 0, formed above) are
    // kept: only the sampled rows are copied out
    const int t0 = std::max(pr->t_first, pr->t_offset == 0 ? 1 : 0);
    for (int k = 0; k < 2; ++k) {
      uint64_t* out = k == 0 ? zbits : xbits;
      if (!out || t0 >= T) continue;
      DTC_HIP(hipMemcpy2DAsync(out + (size_t)bs * row + (size_t)t0 * n_shots,
                               row * sizeof(uint64_t),
                               (k == 0 ? zb : xb) + (size_t)t0 * n_shots, row * sizeof(uint64_t),
                               (size_t)(T - t0) * n_shots * sizeof(uint64_t), (size_t)nb,
                               hipMemcpyDeviceToHost, ctx->stream));
    }
    DTC_HIP(hipStreamSynchronize(ctx->stream));
    DTC_TRY(settle_pending(ctx));
  }
  return DTC_OK;
}

int dtc_sample_draws(uint64_t seed, int64_t traj, int32_t p, int32_t basis, int32_t n_shots,
                     double* u) {
  if (!u) return fail(DTC_EINVAL, "null output");
  if (n_shots < 1 || traj < 0 || p < 0 || basis < 0 || basis > 1)
    return fail(DTC_EINVAL, "dtc_sample_draws: n_shots >= 1, traj >= 0, p >= 0, basis 0 or 1");
  for (int32_t k = 0; k < n_shots; ++k)
    u[k] = dtc::sample_uniform(seed, (uint64_t)traj, (uint32_t)p, (uint32_t)basis, (uint32_t)k);
  return DTC_OK;
}

int dtc_sample_state(const double* state, int32_t L, int32_t basis, const double* u, int32_t n,
                     uint64_t* bits) {
  if (!state || !u || !bits) return fail(DTC_EINVAL, "null argument");
  if (L < 1 || L > 32) return fail(DTC_EINVAL, "L must be in [1, 32]");
  if (n < 1 || basis < 0 || basis > 1) return fail(DTC_EINVAL, "n >= 1, basis 0 or 1");
  const size_t N = (size_t)1 << L;
  std::vector<double> cum(N);
  if (basis == 0) {
    for (size_t x = 0; x < N; ++x)
      cum[x] = state[2 * x] * state[2 * x] + state[2 * x + 1] * state[2 * x + 1];
  } else {
    // H on every site: Walsh-Hadamard butterflies, one factor 2^(-L/2) at the end
    std::vector<double> a(state, state + 2 * N);
    for (size_t h = 1; h < N; h <<= 1)
      for (size_t i = 0; i < N; i += 2 * h)
        for (size_t j = i; j < i + h; ++j)
          for (int c = 0; c < 2; ++c) {
            const double p0 = a[2 * j + c], p1 = a[2 * (j + h) + c];
            a[2 * j + c] = p0 + p1;
            a[2 * (j + h) + c] = p0 - p1;
          }
    const double f = std::ldexp(1.0, -L);
    for (size_t x = 0; x < N; ++x) cum[x] = f * (a[2 * x] * a[2 * x] + a[2 * x + 1] * a[2 * x + 1]);
  }
  // S in index order; the last index of non-zero weight where u W rounds up to W
  size_t last = 0;
  for (size_t x = 0; x < N; ++x)
    if (cum[x] > 0.0) last = x;
  for (size_t x = 1; x < N; ++x) cum[x] += cum[x - 1];
  const double W = cum[N - 1];
  for (int32_t k = 0; k < n; ++k) {
    if (!(u[k] >= 0.0 && u[k] < 1.0)) return fail(DTC_EINVAL, "uniforms must lie in [0, 1)");
    const size_t x = (size_t)(std::upper_bound(cum.begin(), cum.end(), u[k] * W) - cum.begin());
    bits[k] = (uint64_t)(x < N ? x : last);
  }
  return DTC_OK;
}

namespace {

// The two correlator launches on a batch's states `st` (F, or E = H^L F) for
// time row t of out [batch][T][L + L (L - 1) / 2] (per time: the sites, then
// the pairs).  Booked under DTC_KERNEL_REDUCE: the chunk kernel with the
// batch's 16 B per amplitude, the reduce with the chunk partials and its rows.
int launch_corr(dtc_ctx* ctx, const RunCfg& rc, int batch, const double2* st, int t, double* out) {
  const int L = rc.pl.L, n_col = L + dtc::corr::n_pairs(L);
  dtc::CorrArgs A{};
  A.state = st;
  A.partial = (double*)ctx->corr_part.p;
  A.z = out + (size_t)t * n_col;
  A.zz = A.z + L;
  A.out_stride = (int64_t)rc.prob->T * n_col;
  A.L = L;
  A.L_eff = rc.pl.L_eff;
  A.octet_bits = rc.octet_bits;
  A.batch = batch;
  DTC_TIMED(ctx, DTC_KERNEL_REDUCE, 16.0 * (double)rc.pl.len * batch,
            dtc::launch_corr_chunk(A, ctx->stream));
  DTC_TIMED(ctx, DTC_KERNEL_REDUCE,
            8.0 * batch * ((double)rc.pl.n_tiles * dtc::corr::kPartial + n_col),
            dtc::launch_corr_reduce(A, ctx->stream));
  return DTC_OK;
}

// Row p = 0 of one trajectory from its prepared mask m: Z_i = z_i(m),
// C_ij = z_i(m) z_j(m), added to zo [L] and zzo [L (L - 1) / 2] (either may be null).
void corr_basis_row(uint64_t m, int L, double* zo, double* zzo) {
  for (int i = 0; i < L; ++i) {
    if (zo) zo[i] += ((m >> i) & 1ull) ? -1.0 : 1.0;
    if (!zzo) continue;
    for (int j = i + 1; j < L; ++j)
      zzo[dtc::corr::pair_index(L, i, j)] += (((m >> i) ^ (m >> j)) & 1ull) ? -1.0 : 1.0;
  }
}

// sums: the outputs are per-instance sums over the trajectories ([n_inst][T][.],
// dtc_correlation_sums) instead of per-trajectory rows
int corr_impl(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz, uint64_t seed,
              int64_t traj_offset, int32_t n_traj, double* z, double* zz, double* x, double* xx,
              bool sums) {
  if (!ctx || (!z && !zz && !x && !xx)) return fail(DTC_EINVAL, "null ctx/outputs");
  DTC_TRY(check_problem(pr, nz));
  RunCfg rc;
  DTC_TRY(init_run_cfg(ctx, pr, nz, nullptr, nullptr, seed, traj_offset, n_traj, false, rc));
  const Plan& pl = rc.pl;
  const int T = pr->T, L = pr->L;
  const int P = T - 1 + pr->t_offset;
  const int n_pair = dtc::corr::n_pairs(L), n_col = L + n_pair;
  const int64_t S = (int64_t)pr->n_inst * n_traj;
  const bool want_z = z || zz, want_x = x || xx;
  double* const outs[4] = {z, zz, x, xx};
  const size_t n_rows = (size_t)(sums ? pr->n_inst : S) * T;
  for (int k = 0; k < 4; ++k)
    if (outs[k]) std::fill(outs[k], outs[k] + n_rows * ((k & 1) ? n_pair : L), 0.0);

  // Row p = 0: the prepared basis state |m>; every X and XX entry is 0.
  if (pr->t_offset == 0 && pr->t_first == 0) {
    for (int64_t s = 0; s < S; ++s) {
      const uint64_t m = init_state_mask(rc, (uint64_t)(traj_offset + s % n_traj));
      const size_t r = (size_t)(sums ? s / n_traj : s) * T;
      corr_basis_row(m, L, z ? z + r * L : nullptr, zz ? zz + r * n_pair : nullptr);
    }
  }
  if (P == 0) return DTC_OK;
  DTC_TRY(upload_tables(ctx, pr, pl));

  // (the rows of a batch: at most 1 GiB)
  const size_t row = (size_t)T * n_col;  // values per state and basis
  const double per_state = (double)pl.len * 16.0 * (want_x ? 2.0 : 1.0);
  Batch bt;
  DTC_TRY(plan_batch(ctx, rc, per_state, ctx->F.n + (want_x ? ctx->E.n : 0), false,
                     std::max<int64_t>(1, (int64_t)((size_t)(1u << 26) / row)), want_x, -1, bt));
  const int64_t B = bt.B;
  DTC_TRY(ensure(ctx->corr_part, (size_t)B * pl.n_tiles * dtc::corr::kPartial * sizeof(double)));
  DTC_TRY(ensure(ctx->vals_f, 2 * (size_t)B * row * sizeof(double)));
  // per-instance sums: at most (B - 1) / n_traj + 2 instances per batch
  const int64_t max_inst_b = std::min<int64_t>(pr->n_inst, (B - 1) / n_traj + 2);
  const size_t n_host = (size_t)(sums ? max_inst_b : B) * row;  // per basis
  if (sums) DTC_TRY(ensure(ctx->vals_e, 2 * n_host * sizeof(double)));
  DTC_TRY(ensure_host(ctx->host_f, 2 * n_host));
  double* const hv = ctx->host_f.p;
  std::vector<int64_t> masks(B);

  // the schedule (build_sample_schedule, dtc_schedule.h) is the same for every
  // batch; the state a pass leaves at a time is measured in Z on F, in X on
  // E = H^L F
  double2* const F = (double2*)ctx->F.p;
  double* const zv = (double*)ctx->vals_f.p;
  double* const xv = zv + (size_t)B * row;
  std::vector<Launch> sched = build_sample_schedule(rc, F);
  // rows the device does not write (t < t_first, and p = 0, formed above)
  const int t0 = std::max(pr->t_first, pr->t_offset == 0 ? 1 : 0);

  for (int64_t bs = 0; bs < S; bs += B) {
    const int nb = (int)std::min<int64_t>(B, S - bs);
    DTC_TRY(batch_masks(ctx, rc, bs, nb, masks));
    DTC_TRY(basis_source(ctx, sched, F, pl.len, nb, bt.octet));
    DTC_HIP(hipMemsetAsync(zv, 0, 2 * (size_t)B * row * sizeof(double), ctx->stream));
    const AfterLaunch measure = [&](const Launch& l) -> int {
      if (want_z) DTC_TRY(launch_corr(ctx, rc, nb, F, l.t_state, zv));
      if (!want_x) return DTC_OK;
      double2* E = (double2*)ctx->E.p;
      DTC_TRY(launch_xbasis(ctx, rc, bs, nb, F, E, false));
      return launch_corr(ctx, rc, nb, E, l.t_state, xv);
    };
    DTC_TRY(run_launches(ctx, rc, bs, nb, sched, measure));
    // the batch's rows, or their sums per instance (traj_sum_kernel), per basis
    const int64_t i0 = bs / n_traj, n_ib = (bs + nb - 1) / n_traj - i0 + 1;
    const size_t n_get = (size_t)(sums ? n_ib : nb) * row;
    for (int k = 0; k < 2; ++k) {
      if (!(k == 0 ? want_z : want_x)) continue;
      const double* src = k == 0 ? zv : xv;
      if (sums) {
        double* dsum = (double*)ctx->vals_e.p + (size_t)k * n_host;
        DTC_HIP(dtc::launch_traj_sum(src, nb, (int)row, bs, n_traj, dsum, ctx->stream));
        src = dsum;
      }
      DTC_HIP(hipMemcpyAsync(hv + (size_t)k * n_host, src, n_get * sizeof(double),
                             hipMemcpyDeviceToHost, ctx->stream));
    }
    DTC_HIP(hipStreamSynchronize(ctx->stream));
    DTC_TRY(settle_pending(ctx));
    const int64_t n_r = sums ? n_ib : nb, r0 = sums ? i0 : bs;
    for (int k = 0; k < 2; ++k) {
      double* const so = outs[2 * k];       // sites
      double* const po = outs[2 * k + 1];   // pairs
      if (!so && !po) continue;
      for (int64_t r = 0; r < n_r; ++r)
        for (int t = t0; t < T; ++t) {
          const double* v = hv + (size_t)k * n_host + ((size_t)r * T + t) * n_col;
          const size_t o = (size_t)(r0 + r) * T + t;
          // (sums: an instance's trajectories may span batches)
          if (so)
            for (int i = 0; i < L; ++i) so[o * L + i] += v[i];
          if (po)
            for (int i = 0; i < n_pair; ++i) po[o * n_pair + i] += v[L + i];
        }
    }
  }
  return DTC_OK;
}

}  // namespace

int dtc_correlations(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz, uint64_t seed,
                     int64_t traj_offset, int32_t n_traj, double* z, double* zz, double* x,
                     double* xx) {
  return corr_impl(ctx, pr, nz, seed, traj_offset, n_traj, z, zz, x, xx, false);
}

int dtc_correlation_sums(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz, uint64_t seed,
                         int64_t traj_offset, int32_t n_traj, double* z_sum, double* zz_sum,
                         double* x_sum, double* xx_sum) {
  return corr_impl(ctx, pr, nz, seed, traj_offset, n_traj, z_sum, zz_sum, x_sum, xx_sum, true);
}

int dtc_correlations_state(const double* state, int32_t L, int32_t basis, double* z, double* zz) {
  namespace cr = dtc::corr;
  if (!state || !z || (!zz && L > 1)) return fail(DTC_EINVAL, "null argument");
  if (L < 1 || L > 32) return fail(DTC_EINVAL, "L must be in [1, 32]");
  if (basis < 0 || basis > 1) return fail(DTC_EINVAL, "basis 0 or 1");
  const size_t N = (size_t)1 << L;
  const int L_eff = std::max<int>(L, cr::kChunkBits);
  const size_t chunk = (size_t)1 << cr::kChunkBits, n_chunks = (size_t)1 << (L_eff - cr::kChunkBits);
  std::vector<double> w(chunk * n_chunks, 0.0);  // |a|^2, the padding of L < 12 is 0
  if (basis == 0) {
    for (size_t y = 0; y < N; ++y)
      w[y] = state[2 * y] * state[2 * y] + state[2 * y + 1] * state[2 * y + 1];
  } else {
    // H on every site: Walsh-Hadamard butterflies, one factor 2^(-L/2) at the end
    std::vector<double> a(state, state + 2 * N);
    for (size_t h = 1; h < N; h <<= 1)
      for (size_t i = 0; i < N; i += 2 * h)
        for (size_t j = i; j < i + h; ++j)
          for (int c = 0; c < 2; ++c) {
            const double p0 = a[2 * j + c], p1 = a[2 * (j + h) + c];
            a[2 * j + c] = p0 + p1;
            a[2 * (j + h) + c] = p0 - p1;
          }
    const double f = std::ldexp(1.0, -L);
    for (size_t y = 0; y < N; ++y) w[y] = f * (a[2 * y] * a[2 * y] + a[2 * y + 1] * a[2 * y + 1]);
  }
  // the chunk partials as the chunk kernel splits them: per wave (chunk bits 6,
  // 7) the kept coefficients of the other ten bits by plain loops, then the four
  // waves combined
  std::vector<double> part(n_chunks * cr::kPartial);
  for (size_t c = 0; c < n_chunks; ++c) {
    double sv[4][cr::kWaveSlots];
    for (int m = 0; m < (int)chunk; ++m) {
      const int slot = cr::slot_of_mask(m);
      if (slot < 0) continue;
      for (int wv = 0; wv < 4; ++wv) {
        double acc = 0.0;
        for (int y = 0; y < (int)chunk; ++y)
          if (((y >> 6) & 3) == wv)
            acc += __builtin_parity((unsigned)(y & m)) ? -w[c * chunk + y] : w[c * chunk + y];
        sv[wv][slot] = acc;
      }
    }
    for (int o = 0; o < cr::kPartial; ++o) {
      const int m = cr::partial_mask(o);
      const int slot = cr::slot_of_mask(m & ~cr::kWaveBitMask);
      part[c * cr::kPartial + o] =
          cr::wave_combine((m >> 6) & 3, sv[0][slot], sv[1][slot], sv[2][slot], sv[3][slot]);
    }
  }
  const int n_out = L + cr::n_pairs(L);
  for (int o = 0; o < n_out; ++o) {
    const cr::Source src = cr::output_source(L, o);
    double acc = 0.0;
    for (size_t c = 0; c < n_chunks; ++c) acc += cr::term(&part[c * cr::kPartial], src, c);
    (o < L ? z[o] : zz[o - L]) = acc;
  }
  return DTC_OK;
}

namespace {

// The two launches of one window on a batch's states F: the matrices go to
// out[b * out_stride ..].  Booked under DTC_KERNEL_REDUCE: the Gram kernel with
// the batch's 16 B per amplitude, the reduce with the partials and its rows.
int launch_rdm(dtc_ctx* ctx, const RunCfg& rc, int batch, const double2* st,
               const dtc::rdm::Geom& g, double* out, int64_t out_stride) {
  dtc::RdmArgs A{};
  A.state = st;
  A.partial = (double*)ctx->rdm_part.p;
  A.out = out;
  A.out_stride = out_stride;
  A.L_eff = rc.pl.L_eff;
  A.octet_bits = rc.octet_bits;
  A.batch = batch;
  A.g = g;
  DTC_TIMED(ctx, DTC_KERNEL_REDUCE, 16.0 * (double)rc.pl.len * batch,
            dtc::launch_rdm_gram(A, ctx->stream));
  DTC_TIMED(ctx, DTC_KERNEL_REDUCE,
            8.0 * batch *
                ((double)dtc::rdm::n_workgroups(rc.pl.L_eff) * dtc::rdm::kPartial +
                 (double)((size_t)2 << (2 * g.k))),
            dtc::launch_rdm_reduce(A, ctx->stream));
  return DTC_OK;
}

int check_windows(const int32_t* sites, int32_t n_win, int32_t k, int L) {
  if (!sites) return fail(DTC_EINVAL, "null sites");
  if (n_win < 1) return fail(DTC_EINVAL, "n_win must be >= 1");
  if (k < 1 || k > dtc::rdm::kMaxK) return fail(DTC_EINVAL, "window size k must be in [1, 4]");
  for (int32_t w = 0; w < n_win; ++w)
    if (const char* err = dtc::rdm::check_window(sites + (size_t)w * k, k, L))
      return fail(DTC_EINVAL, err);
  return DTC_OK;
}

// sums: rho is the per-instance sum over the trajectories ([n_inst][T][.],
// dtc_rdm_sums) instead of per-trajectory rows
int rdm_impl(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz, uint64_t seed,
             int64_t traj_offset, int32_t n_traj, const int32_t* sites, int32_t n_win, int32_t k,
             double* rho, bool sums) {
  if (!ctx || !rho) return fail(DTC_EINVAL, "null ctx/output");
  DTC_TRY(check_problem(pr, nz));
  DTC_TRY(check_windows(sites, n_win, k, pr->L));
  RunCfg rc;
  DTC_TRY(init_run_cfg(ctx, pr, nz, nullptr, nullptr, seed, traj_offset, n_traj, false, rc));
  const Plan& pl = rc.pl;
  const int T = pr->T;
  const int P = T - 1 + pr->t_offset;
  const int64_t S = (int64_t)pr->n_inst * n_traj;
  const size_t mat = (size_t)2 << (2 * k);         // doubles per matrix: d d 2
  const size_t row = (size_t)T * n_win * mat;      // doubles per state
  const size_t n_rows = (size_t)(sums ? pr->n_inst : S);
  if ((double)T * n_win * (double)mat > (double)(1u << 26))
    return fail(DTC_EINVAL, "T n_win d d exceeds 2^25 matrix entries per state");
  std::fill(rho, rho + n_rows * row, 0.0);

  // Row p = 0: the prepared basis state |m>, rho = |m_A><m_A|.
  if (pr->t_offset == 0 && pr->t_first == 0) {
    for (int64_t s = 0; s < S; ++s) {
      const uint64_t m = init_state_mask(rc, (uint64_t)(traj_offset + s % n_traj));
      double* r = rho + (size_t)(sums ? s / n_traj : s) * row;
      for (int32_t w = 0; w < n_win; ++w) {
        size_t al = 0;
        for (int i = 0; i < k; ++i) al |= (size_t)((m >> sites[(size_t)w * k + i]) & 1ull) << i;
        r[(size_t)w * mat + 2 * ((al << k) + al)] += 1.0;
      }
    }
  }
  if (P == 0) return DTC_OK;
  DTC_TRY(upload_tables(ctx, pr, pl));

  std::vector<dtc::rdm::Geom> geo((size_t)n_win);
  for (int32_t w = 0; w < n_win; ++w)
    geo[w] = dtc::rdm::geometry(sites + (size_t)w * k, k, pl.L_eff);

  // (the rows of a batch: at most 512 MiB)
  const double per_state = (double)pl.len * 16.0;
  Batch bt;
  DTC_TRY(plan_batch(ctx, rc, per_state, ctx->F.n, false,
                     std::max<int64_t>(1, (int64_t)((size_t)(1u << 26) / row)), false, -1, bt));
  const int64_t B = bt.B;
  DTC_TRY(ensure(ctx->rdm_part, (size_t)B * (size_t)dtc::rdm::n_workgroups(pl.L_eff) *
                                    dtc::rdm::kPartial * sizeof(double)));
  DTC_TRY(ensure(ctx->vals_f, (size_t)B * row * sizeof(double)));
  // per-instance sums: at most (B - 1) / n_traj + 2 instances per batch
  const int64_t max_inst_b = std::min<int64_t>(pr->n_inst, (B - 1) / n_traj + 2);
  const size_t n_host = (size_t)(sums ? max_inst_b : B) * row;
  if (sums) DTC_TRY(ensure(ctx->vals_e, n_host * sizeof(double)));
  DTC_TRY(ensure_host(ctx->host_f, n_host));
  double* const hv = ctx->host_f.p;
  std::vector<int64_t> masks(B);

  // the schedule (build_sample_schedule, dtc_schedule.h) is the same for every
  // batch; the state a pass leaves at a time is read once per window
  double2* const F = (double2*)ctx->F.p;
  double* const rv = (double*)ctx->vals_f.p;
  std::vector<Launch> sched = build_sample_schedule(rc, F);
  // rows the device does not write (t < t_first, and p = 0, formed above)
  const int t0 = std::max(pr->t_first, pr->t_offset == 0 ? 1 : 0);

  for (int64_t bs = 0; bs < S; bs += B) {
    const int nb = (int)std::min<int64_t>(B, S - bs);
    DTC_TRY(batch_masks(ctx, rc, bs, nb, masks));
    DTC_TRY(basis_source(ctx, sched, F, pl.len, nb, bt.octet));
    DTC_HIP(hipMemsetAsync(rv, 0, (size_t)B * row * sizeof(double), ctx->stream));
    const AfterLaunch measure = [&](const Launch& l) -> int {
      for (int32_t w = 0; w < n_win; ++w)
        DTC_TRY(launch_rdm(ctx, rc, nb, F, geo[w],
                           rv + ((size_t)l.t_state * n_win + w) * mat, (int64_t)row));
      return DTC_OK;
    };
    DTC_TRY(run_launches(ctx, rc, bs, nb, sched, measure));
    // the batch's rows, or their sums per instance (traj_sum_kernel)
    const int64_t i0 = bs / n_traj, n_ib = (bs + nb - 1) / n_traj - i0 + 1;
    const size_t n_get = (size_t)(sums ? n_ib : nb) * row;
    const double* src = rv;
    if (sums) {
      double* dsum = (double*)ctx->vals_e.p;
      DTC_HIP(dtc::launch_traj_sum(src, nb, (int)row, bs, n_traj, dsum, ctx->stream));
      src = dsum;
    }
    DTC_HIP(hipMemcpyAsync(hv, src, n_get * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    DTC_HIP(hipStreamSynchronize(ctx->stream));
    DTC_TRY(settle_pending(ctx));
    const int64_t n_r = sums ? n_ib : nb, r0 = sums ? i0 : bs;
    const size_t per_t = (size_t)n_win * mat;
    for (int64_t r = 0; r < n_r; ++r) {
      // (sums: an instance's trajectories may span batches)
      const double* v = hv + (size_t)r * row;
      double* o = rho + (size_t)(r0 + r) * row;
      for (size_t i = (size_t)t0 * per_t; i < row; ++i) o[i] += v[i];
    }
  }
  return DTC_OK;
}

}  // namespace

int dtc_rdm(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz, uint64_t seed,
            int64_t traj_offset, int32_t n_traj, const int32_t* sites, int32_t n_win, int32_t k,
            double* rho) {
  return rdm_impl(ctx, pr, nz, seed, traj_offset, n_traj, sites, n_win, k, rho, false);
}

int dtc_rdm_sums(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz, uint64_t seed,
                 int64_t traj_offset, int32_t n_traj, const int32_t* sites, int32_t n_win,
                 int32_t k, double* rho_sum) {
  return rdm_impl(ctx, pr, nz, seed, traj_offset, n_traj, sites, n_win, k, rho_sum, true);
}

int dtc_rdm_state(const double* state, int32_t L, const int32_t* sites, int32_t k, double* rho) {
  namespace rd = dtc::rdm;
  if (!state || !sites || !rho) return fail(DTC_EINVAL, "null argument");
  if (L < 1 || L > 32) return fail(DTC_EINVAL, "L must be in [1, 32]");
  if (const char* err = rd::check_window(sites, k, L)) return fail(DTC_EINVAL, err);
  const int d = 1 << k;
  int pos[rd::kMaxK];
  uint64_t off[rd::kRows];
  for (int m = 0; m < k; ++m) pos[m] = sites[m];
  for (int a = 0; a < d; ++a) off[a] = rd::row_offset(a, pos, k);
  // the lower triangle by plain sums over the column index in ascending order
  std::vector<double> re((size_t)d * d, 0.0), im((size_t)d * d, 0.0);
  const uint64_t n_cols = (uint64_t)1 << (L - k);
  for (uint64_t c = 0; c < n_cols; ++c) {
    const uint64_t x0 = rd::spread_cols(c, pos, k);
    for (int a = 0; a < d; ++a) {
      const double ar = state[2 * (x0 | off[a])], ai = state[2 * (x0 | off[a]) + 1];
      for (int a2 = 0; a2 <= a; ++a2) {
        const double br = state[2 * (x0 | off[a2])], bi = state[2 * (x0 | off[a2]) + 1];
        re[(size_t)a * d + a2] += ar * br + ai * bi;
        im[(size_t)a * d + a2] += ai * br - ar * bi;
      }
    }
  }
  for (int a = 0; a < d; ++a)
    for (int a2 = 0; a2 <= a; ++a2) {
      const double gr = re[(size_t)a * d + a2], gi = a == a2 ? 0.0 : im[(size_t)a * d + a2];
      rho[2 * ((size_t)a * d + a2)] = gr;
      rho[2 * ((size_t)a * d + a2) + 1] = gi;
      if (a == a2) continue;
      rho[2 * ((size_t)a2 * d + a)] = gr;
      rho[2 * ((size_t)a2 * d + a) + 1] = -gi;
    }
  return DTC_OK;
}

namespace {

int check_blocks(const int32_t* starts, int32_t n_blk, int32_t k, int L) {
  if (!starts) return fail(DTC_EINVAL, "null starts");
  if (n_blk < 1) return fail(DTC_EINVAL, "n_blk must be >= 1");
  for (int32_t w = 0; w < n_blk; ++w)
    if (const char* err = dtc::rdmb::check_block(starts[w], k, L)) return fail(DTC_EINVAL, err);
  return DTC_OK;
}

}  // namespace

int dtc_rdm_block_sums(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz, uint64_t seed,
                       int64_t traj_offset, int32_t n_traj, const int32_t* starts, int32_t n_blk,
                       int32_t k, double* rho_sum, double* purity) {
  namespace rb = dtc::rdmb;
  if (!ctx || (!rho_sum && !purity)) return fail(DTC_EINVAL, "null ctx/outputs");
  DTC_TRY(check_problem(pr, nz));
  DTC_TRY(check_blocks(starts, n_blk, k, pr->L));
  const int T = pr->T;
  const size_t mat = (size_t)2 << (2 * k);         // doubles per matrix: d d 2
  if ((double)T * n_blk * (double)mat > (double)(1u << 26))
    return fail(DTC_EINVAL, "T n_blk d d exceeds 2^25 matrix entries per instance");
  RunCfg rc;
  DTC_TRY(init_run_cfg(ctx, pr, nz, nullptr, nullptr, seed, traj_offset, n_traj, false, rc));
  const Plan& pl = rc.pl;
  const int P = T - 1 + pr->t_offset;
  const int64_t S = (int64_t)pr->n_inst * n_traj;
  const size_t row = (size_t)T * n_blk * mat;      // doubles per instance
  const size_t prow = (size_t)T * n_blk;           // purities per state
  if (rho_sum) std::fill(rho_sum, rho_sum + (size_t)pr->n_inst * row, 0.0);
  if (purity) std::fill(purity, purity + (size_t)S * prow, 0.0);

  // Row p = 0: the prepared basis state |m>, rho = |m_A><m_A|, purity 1.
  if (pr->t_offset == 0 && pr->t_first == 0) {
    for (int64_t s = 0; s < S; ++s) {
      const uint64_t m = init_state_mask(rc, (uint64_t)(traj_offset + s % n_traj));
      for (int32_t w = 0; w < n_blk; ++w) {
        const size_t al = (size_t)((m >> starts[w]) & (((uint64_t)1 << k) - 1));
        if (rho_sum)
          rho_sum[(size_t)(s / n_traj) * row + (size_t)w * mat + 2 * ((al << k) + al)] += 1.0;
        if (purity) purity[(size_t)s * prow + w] = 1.0;
      }
    }
  }
  if (P == 0) return DTC_OK;
  DTC_TRY(upload_tables(ctx, pr, pl));

  std::vector<rb::Geom> geo((size_t)n_blk);
  size_t part_doubles = 0;   // per state
  for (int32_t w = 0; w < n_blk; ++w) {
    geo[w] = rb::geometry(starts[w], k, pl.L_eff);
    if (geo[w].n_split > 1 || geo[w].n_pad > 1)
      part_doubles =
          std::max(part_doubles, (size_t)geo[w].n_split * ((size_t)2 << (2 * geo[w].ke)));
  }

  // A batch holds at most max_inst instances' sums ([T][n_blk][.][d][d][2], at
  // most 2^28 doubles), which caps its states; the states, their matrices and
  // partials and their share of the sums count against the memory budget.
  const int64_t max_inst_cap = std::max<int64_t>(4, (int64_t)(((size_t)1 << 28) / row));
  const int64_t cap_B = rho_sum ? (max_inst_cap - 2) * (int64_t)n_traj + 1 : 0;
  const double per_state = (double)pl.len * 16.0 + 8.0 * (double)(mat + part_doubles) +
                           (rho_sum ? 8.0 * (double)row / n_traj : 0.0);
  Batch bt;
  DTC_TRY(plan_batch(ctx, rc, per_state, ctx->F.n, false, cap_B, false, -1, bt));
  const int64_t B = bt.B;
  const int64_t max_inst_b = std::min<int64_t>(pr->n_inst, (B - 1) / n_traj + 2);
  DTC_TRY(ensure(ctx->rdmb_work, (size_t)B * mat * sizeof(double)));
  if (part_doubles) DTC_TRY(ensure(ctx->rdmb_part, (size_t)B * part_doubles * sizeof(double)));
  DTC_TRY(ensure(ctx->vals_f, (size_t)B * prow * sizeof(double)));
  const size_t sum_doubles = (size_t)max_inst_b * row;
  if (rho_sum) DTC_TRY(ensure(ctx->rdmb_sum, sum_doubles * sizeof(double)));
  DTC_TRY(ensure_host(ctx->host_f, (rho_sum ? sum_doubles : 0) + (size_t)B * prow));
  double* const hs = ctx->host_f.p;
  double* const hp = hs + (rho_sum ? sum_doubles : 0);
  std::vector<int64_t> masks(B);

  double2* const F = (double2*)ctx->F.p;
  double* const pv = (double*)ctx->vals_f.p;
  double* const dsum = (double*)ctx->rdmb_sum.p;
  std::vector<Launch> sched = build_sample_schedule(rc, F);
  // rows the device does not write (t < t_first, and p = 0, formed above)
  const int t0 = std::max(pr->t_first, pr->t_offset == 0 ? 1 : 0);

  for (int64_t bs = 0; bs < S; bs += B) {
    const int nb = (int)std::min<int64_t>(B, S - bs);
    const int64_t i0 = bs / n_traj, n_ib = (bs + nb - 1) / n_traj - i0 + 1;
    DTC_TRY(batch_masks(ctx, rc, bs, nb, masks));
    DTC_TRY(basis_source(ctx, sched, F, pl.len, nb, bt.octet));
    DTC_HIP(hipMemsetAsync(pv, 0, (size_t)B * prow * sizeof(double), ctx->stream));
    const AfterLaunch measure = [&](const Launch& l) -> int {
      for (int32_t w = 0; w < n_blk; ++w) {
        const rb::Geom& g = geo[w];
        const size_t slot = (size_t)l.t_state * n_blk + w;
        dtc::RdmBlockArgs A{};
        A.state = F;
        A.partial = (double*)ctx->rdmb_part.p;
        A.work = (double*)ctx->rdmb_work.p;
        A.work_stride = (int64_t)mat;
        A.purity = pv + slot;
        A.purity_stride = (int64_t)prow;
        A.L_eff = pl.L_eff;
        A.octet_bits = rc.octet_bits;
        A.batch = nb;
        A.g = g;
        const bool direct = g.n_split == 1 && g.n_pad == 1;
        if (direct) A.partial = A.work;  // (unused)
        // the Gram launch reads a panel pair per tile; booked with the batch's
        // 16 B per amplitude plus the matrices written
        DTC_TIMED(ctx, DTC_KERNEL_REDUCE,
                  16.0 * (double)pl.len * nb + 8.0 * nb * (double)mat,
                  dtc::launch_rdm_block_gram(A, ctx->stream));
        if (purity) {
          DTC_TIMED(ctx, DTC_KERNEL_REDUCE, 8.0 * nb * (double)(mat + 1),
                    dtc::launch_rdm_block_purity(A, ctx->stream));
        }
        if (rho_sum) {
          DTC_TIMED(ctx, DTC_KERNEL_REDUCE, 8.0 * (double)(nb + n_ib) * (double)mat,
                    dtc::launch_traj_sum(A.work, nb, (int)mat, bs, n_traj,
                                         dsum + slot * (size_t)max_inst_b * mat, ctx->stream));
        }
      }
      return DTC_OK;
    };
    DTC_TRY(run_launches(ctx, rc, bs, nb, sched, measure));
    if (rho_sum)
      DTC_HIP(hipMemcpyAsync(hs, dsum, sum_doubles * sizeof(double), hipMemcpyDeviceToHost,
                             ctx->stream));
    if (purity)
      DTC_HIP(hipMemcpyAsync(hp, pv, (size_t)nb * prow * sizeof(double), hipMemcpyDeviceToHost,
                             ctx->stream));
    DTC_HIP(hipStreamSynchronize(ctx->stream));
    DTC_TRY(settle_pending(ctx));
    if (rho_sum)
      for (int t = t0; t < T; ++t)
        for (int32_t w = 0; w < n_blk; ++w) {
          const size_t slot = (size_t)t * n_blk + w;
          for (int64_t r = 0; r < n_ib; ++r) {
            // (an instance's trajectories may span batches)
            const double* v = hs + (slot * (size_t)max_inst_b + (size_t)r) * mat;
            double* o = rho_sum + (size_t)(i0 + r) * row + slot * mat;
            for (size_t i = 0; i < mat; ++i) o[i] += v[i];
          }
        }
    if (purity)
      for (int b = 0; b < nb; ++b)
        for (size_t i = (size_t)t0 * n_blk; i < prow; ++i)
          purity[(size_t)(bs + b) * prow + i] = hp[(size_t)b * prow + i];
  }
  return DTC_OK;
}

int dtc_rdm_block_state(const double* state, int32_t L, int32_t start, int32_t k, double* rho,
                        double* purity) {
  namespace rb = dtc::rdmb;
  if (!state || !purity) return fail(DTC_EINVAL, "null argument");
  if (const char* err = rb::check_block(start, k, L)) return fail(DTC_EINVAL, err);
  const size_t d = (size_t)1 << k;
  // the block's own bits are the row: no pad on the host (ke = k, ae = start)
  std::vector<double> re(d * d, 0.0), im(d * d, 0.0), vr(d), vi(d);
  const uint64_t n_cols = (uint64_t)1 << (L - k);
  // the lower triangle by plain sums over the column index in ascending order
  for (uint64_t c = 0; c < n_cols; ++c) {
    for (size_t a = 0; a < d; ++a) {
      const uint64_t x = rb::amp_index(start, k, a, c);
      vr[a] = state[2 * x];
      vi[a] = state[2 * x + 1];
    }
    for (size_t a = 0; a < d; ++a) {
      const double ar = vr[a], ai = vi[a];
      double* rr = &re[a * d];
      double* ri = &im[a * d];
      for (size_t a2 = 0; a2 <= a; ++a2) {
        rr[a2] += ar * vr[a2] + ai * vi[a2];
        ri[a2] += ai * vr[a2] - ar * vi[a2];
      }
    }
  }
  double pur = 0.0;
  for (size_t a = 0; a < d; ++a)
    for (size_t a2 = 0; a2 <= a; ++a2) {
      const double gr = re[a * d + a2], gi = a == a2 ? 0.0 : im[a * d + a2];
      pur += (a == a2 ? 1.0 : 2.0) * (gr * gr + gi * gi);
      if (!rho) continue;
      rho[2 * (a * d + a2)] = gr;
      rho[2 * (a * d + a2) + 1] = gi;
      if (a == a2) continue;
      rho[2 * (a2 * d + a)] = gr;
      rho[2 * (a2 * d + a) + 1] = -gi;
    }
  *purity = pur;
  return DTC_OK;
}

int32_t dtc_plan_groups(int32_t n_bits, uint64_t* masks, int32_t max_groups) {
  if (n_bits < 1 || n_bits > 40 || !masks) return fail(DTC_EINVAL, "bad arguments");
  Plan pl = make_plan(n_bits, true);
  if ((int)pl.groups.size() > max_groups) return fail(DTC_EINVAL, "max_groups too small");
  for (size_t g = 0; g < pl.groups.size(); ++g)
    masks[g] = group_bits(pl.groups[g]) & ((n_bits >= 64) ? ~0ull : ((1ull << n_bits) - 1));
  return (int32_t)pl.groups.size();
}

int dtc_shard_set_basis(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz,
                        const dtc_shard* sh, uint64_t seed, int64_t traj, double* state) {
  if (!ctx || !state) return fail(DTC_EINVAL, "null ctx/state");
  DTC_TRY(check_problem(pr, nz, 64));
  DTC_TRY(check_shard(pr, sh));
  if (traj < 0) return fail(DTC_EINVAL, "traj must be >= 0");
  DTC_HIP(hipSetDevice(ctx->device));
  uint64_t mask = pr->init_mask;
  if (nz->p > 0.0) {  // as init_state_mask: X/Y errors after a prep X undo the flip
    uint32_t t1, t2, t3;
    thresholds(nz->p, &t1, &t2, &t3);
    for (int i = 0; i < pr->L; ++i) {
      if (!((pr->init_mask >> i) & 1ull)) continue;
      const int pz = dtc::sample_pauli(seed, (uint64_t)traj, dtc::kStreamPrep, 0u, (uint32_t)i,
                                       0u, t1, t2, t3);
      if (pz == 1 || pz == 2) mask &= ~(1ull << i);
    }
  }
  const int nl = sh->n_local;
  const size_t len = (size_t)1 << nl;
  DTC_HIP(hipMemsetAsync(state, 0, len * 16 * sh->n_shards, ctx->stream));
  uint64_t local = 0, rank = 0;
  for (int q = 0; q < pr->L; ++q) {
    const uint64_t bit = (mask >> sh->site_of[q]) & 1;
    if (q < nl) local |= bit << q;
    else rank |= bit << (q - nl);
  }
  const int64_t b = (int64_t)rank - sh->first_rank;
  static const double one[2] = {1.0, 0.0};
  if (b >= 0 && b < sh->n_shards)
    DTC_HIP(hipMemcpyAsync(state + 2 * ((size_t)b * len + local), one, 16,
                           hipMemcpyHostToDevice, ctx->stream));
  DTC_HIP(hipStreamSynchronize(ctx->stream));
  return DTC_OK;
}

}  // extern "C"

namespace {

uint64_t fnv(uint64_t h, const void* p, size_t n) {
  const unsigned char* c = (const unsigned char*)p;
  for (size_t i = 0; i < n; ++i) h = (h ^ c[i]) * 1099511628211ull;
  return h;
}

// A small device-table cache (most recent last, at most 4 entries): the entry
// for `key`, built by `fill` (host bytes) on a miss.  Evicting an entry waits
// for the stream (its table may be in use); a sweep alternates two bit maps,
// so that happens only when a caller switches problems.
template <class Fill>
int cached_table(dtc_ctx* ctx, std::vector<dtc_ctx::ShardTables>& cache, uint64_t key,
                 Fill fill, const void** out) {
  for (auto& e : cache)
    if (e.key == key) {
      *out = e.diag.p;
      return DTC_OK;
    }
  std::vector<double> host;
  fill(host);
  if (cache.size() >= 4) {
    DTC_HIP(hipStreamSynchronize(ctx->stream));
    release(cache.front().diag);
    cache.erase(cache.begin());
  }
  cache.emplace_back();
  auto& e = cache.back();
  DTC_TRY(ensure(e.diag, host.size() * sizeof(double)));
  DTC_HIP(hipMemcpy(e.diag.p, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice));
  e.key = key;
  *out = e.diag.p;
  return DTC_OK;
}

// The kick-side tables of a shard bit map: the bit -> site map (cached per
// map) and the logical kick table.  dtc_shard_kick_slice needs only these.
int shard_kick_tables(dtc_ctx* ctx, const dtc_problem* pr, const dtc_shard* sh, RunCfg& rc) {
  const int L = pr->L;
  const int n_rows = std::max(1, pr->T - 1 + pr->t_offset);
  uint64_t mkey = fnv(1469598103934665603ull, sh->site_of, sizeof(int32_t) * 64);
  const void* map = nullptr;
  DTC_TRY(cached_table(ctx, ctx->shard_maps, mkey,
                       [&](std::vector<double>& h) {
                         h.assign(32, 0.0);  // 64 int32 in 32 doubles
                         std::memcpy(h.data(), sh->site_of, 64 * sizeof(int32_t));
                       },
                       &map));
  rc.site_of = (const int*)map;
  const size_t kb = (size_t)n_rows * L * pr->n_sub * 8 * sizeof(double);
  uint64_t kkey = fnv(1469598103934665603ull, &kb, sizeof(kb));
  kkey = fnv(kkey, pr->kick, kb);
  if (kkey != ctx->shard_kick_key || !ctx->shard_kick.p) {
    DTC_HIP(hipStreamSynchronize(ctx->stream));  // the previous table may be in use
    DTC_TRY(ensure(ctx->shard_kick, kb));
    DTC_HIP(hipMemcpy(ctx->shard_kick.p, pr->kick, kb, hipMemcpyHostToDevice));
    ctx->shard_kick_key = kkey;
  }
  rc.kick_tab = (const double2*)ctx->shard_kick.p;
  return DTC_OK;
}

// Device tables of one shard bit map and instance: the effective diagonal per
// held shard (cached per map, instance and angles) plus the kick-side tables.
int shard_tables(dtc_ctx* ctx, const dtc_problem* pr, const dtc_shard* sh, int inst,
                 const Plan& pl, RunCfg& rc) {
  const int L = pr->L, nl = sh->n_local, B = sh->n_shards;
  uint64_t key = 1469598103934665603ull;
  key = fnv(key, &L, sizeof(L));
  key = fnv(key, &sh->n_local, sizeof(int32_t) * 4);
  key = fnv(key, sh->site_of, sizeof(int32_t) * L);
  key = fnv(key, &inst, sizeof(inst));
  key = fnv(key, pr->h + (size_t)inst * L, sizeof(double) * L);
  if (L > 1) key = fnv(key, pr->phi + (size_t)inst * (L - 1), sizeof(double) * (L - 1));
  const void* tab = nullptr;
  DTC_TRY(cached_table(ctx, ctx->shard_cache, key,
                       [&](std::vector<double>& dt) {
                         std::vector<double> he((size_t)B * nl),
                             pe((size_t)B * std::max(nl - 1, 1)), ca(B);
                         for (int b = 0; b < B; ++b)
                           shard_chain(pr, sh, inst, sh->first_rank + b,
                                       he.data() + (size_t)b * nl,
                                       pe.data() + (size_t)b * std::max(nl - 1, 1), &ca[b]);
                         build_diag_tables(pl, B, he.data(), pe.data(), dt, ca.data());
                       },
                       &tab));
  rc.diag_tab = (const double2*)tab;
  return shard_kick_tables(ctx, pr, sh, rc);
}

int shard_check_common(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz,
                       const dtc_shard* sh, int64_t traj, int32_t inst) {
  if (!ctx) return fail(DTC_EINVAL, "null ctx");
  DTC_TRY(check_problem(pr, nz, 64));
  DTC_TRY(check_shard(pr, sh));
  if (inst < 0 || inst >= pr->n_inst) return fail(DTC_EINVAL, "inst out of range");
  if (traj < 0) return fail(DTC_EINVAL, "traj must be >= 0");
  return DTC_OK;
}

RunCfg shard_runcfg(const dtc_problem* pr, const dtc_noise* nz, const dtc_shard* sh,
                    uint64_t seed, int64_t traj) {
  RunCfg rc;
  rc.prob = pr;
  rc.pl = make_plan(sh->n_local, true);
  rc.seed = seed;
  rc.traj_offset = traj;
  rc.n_traj = 1;  // batch index b = shard b -> diag table b
  rc.noisy = nz->p > 0.0 ? 1 : 0;
  rc.row_kind = classify_rows(pr);
  thresholds(nz->p, &rc.thr1, &rc.thr2, &rc.thr3);
  return rc;
}

// A kick layer of a sharded step: kick-table row, KickMode, RNG stream and
// counter (the mask a call gives says which bits take it).
struct ShardLayer {
  int row, mode;
  uint32_t stream, counter;
};
// The layers a step addresses: dst = post . D^diag . pre . src, D in diag_mode.
struct ShardLayers {
  ShardLayer pre, post;
  int diag_mode;
};

// forward: K_period, then D, then K_{period+1} (stream 0, counter = period)
ShardLayer shard_forward_layer(int period) {
  return ShardLayer{period - 1, dtc::kKickForward, dtc::kStreamForward, (uint32_t)period};
}
ShardLayers shard_forward_layers(int period) {
  return ShardLayers{shard_forward_layer(period), shard_forward_layer(period + 1), dtc::kDiagFwd};
}
// echo chain t, layer k (p = t + t_offset; echo_chain's layers in dtc_schedule.h):
// k = 0 the exact undo of the forward layer K_{p+1} that ran ahead, 1 <= k <= p
// the inverse kick K'_k of period p - k + 1 (stream 1 + t, counter k)
ShardLayer shard_echo_layer(int t, int p, int k) {
  if (k == 0) return ShardLayer{p, dtc::kKickUndo, dtc::kStreamForward, (uint32_t)(p + 1)};
  return ShardLayer{p - k, dtc::kKickInverse, (uint32_t)(1 + t), (uint32_t)k};
}
int shard_echo_check(const dtc_problem* pr, int32_t t, int32_t k) {
  if (!pr) return fail(DTC_EINVAL, "null problem");
  if (t < 0 || t >= pr->T) return fail(DTC_EINVAL, "t outside [0, T)");
  if (k < 0 || k > t + pr->t_offset) return fail(DTC_EINVAL, "k outside [0, t + t_offset]");
  return DTC_OK;
}

dtc::KickDesc shard_kick_desc(const ShardLayer& ly, const Group& g, uint64_t mask) {
  return dtc::KickDesc{1, ly.row, ly.mode, ly.stream, ly.counter, skip_bits(g, mask)};
}

// dtc_shard_step / dtc_shard_step_async and their echo twins: obs is a host
// array (copied, then the stream is synchronised) or, when obs_on_device, a
// device array the reduction writes directly (nothing waits).  no_dst_ok (the
// echo twins): dst == NULL runs the chain's end, one kick-only pass that
// measures and stores nothing.
int shard_step_impl(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz,
                    const dtc_shard* sh, uint64_t seed, int64_t traj, int32_t inst,
                    const ShardLayers& ly, uint64_t pre_mask, int32_t diag, uint64_t post_mask,
                    const double* src, double* dst, double* obs, bool obs_on_device,
                    bool no_dst_ok = false) {
  if (!src || (!dst && !no_dst_ok)) return fail(DTC_EINVAL, "null src/dst");
  DTC_TRY(shard_check_common(ctx, pr, nz, sh, traj, inst));
  const int nl = sh->n_local;
  const uint64_t all = nl >= 64 ? ~0ull : (1ull << nl) - 1;
  if ((pre_mask | post_mask) & ~all) return fail(DTC_EINVAL, "kick mask has non-local bits");
  if (post_mask && !diag) return fail(DTC_EINVAL, "post_mask needs diag");
  const int n_rows = std::max(1, pr->T - 1 + pr->t_offset);
  if (pre_mask && (ly.pre.row < 0 || ly.pre.row >= n_rows))
    return fail(DTC_EINVAL, "period outside kick table");
  if (post_mask && (ly.post.row < 0 || ly.post.row >= n_rows))
    return fail(DTC_EINVAL, "period + 1 outside kick table");
  if (!dst && (diag || post_mask || !pre_mask || !obs))
    return fail(DTC_EINVAL, "dst == NULL is the measured kick-only end of a chain");
  DTC_HIP(hipSetDevice(ctx->device));

  RunCfg rc = shard_runcfg(pr, nz, sh, seed, traj);
  const Plan& pl = rc.pl;
  const int B = sh->n_shards;
  if (!dst) {
    int holding = 0;
    for (const Group& g : pl.groups)
      if (pre_mask & group_bits(g)) ++holding;
    if (holding != 1) return fail(DTC_EINVAL, "dst == NULL needs the kicked bits in one site group");
  }
  DTC_TRY(shard_tables(ctx, pr, sh, inst, pl, rc));
  const int n_obs = 1 + nl;
  DTC_TRY(ensure(ctx->partial, (size_t)B * pl.n_tiles * n_obs * sizeof(double)));
  DTC_TRY(ensure(ctx->vals_f, (size_t)B * n_obs * sizeof(double)));
  double* meas_out = obs_on_device ? obs : (double*)ctx->vals_f.p;

  auto layer = [&](const ShardLayer& l, uint64_t mask, const Group& g) {
    return shard_kick_desc(l, g, mask);
  };
  // main group: holds the highest kicked bit (the bits an exchange just made local)
  const uint64_t any = pre_mask | post_mask;
  int main_g = (int)pl.groups.size() - 1;
  if (any) {
    const int top = 63 - __builtin_clzll(any);
    for (size_t g = 0; g < pl.groups.size(); ++g)
      if ((group_bits(pl.groups[g]) >> top) & 1) main_g = (int)g;
  }
  std::vector<PassSpec> passes;
  for (size_t g = 0; g < pl.groups.size(); ++g) {
    const uint64_t gb = group_bits(pl.groups[g]);
    if ((int)g != main_g && (pre_mask & gb))
      passes.push_back(PassSpec{(int)g, layer(ly.pre, pre_mask, pl.groups[g]), no_kick(),
                                dtc::kDiagNone, 0});
  }
  const Group& mg = pl.groups[main_g];
  const uint64_t mb = group_bits(mg);
  PassSpec mp{main_g, no_kick(), no_kick(), diag ? ly.diag_mode : dtc::kDiagNone, 1};
  if (pre_mask & mb) mp.pre = layer(ly.pre, pre_mask, mg);
  if (post_mask & mb) mp.post = layer(ly.post, post_mask, mg);
  const int main_idx = (int)passes.size();
  if (mp.pre.enabled || mp.post.enabled || diag) passes.push_back(mp);
  const int meas_idx = diag ? main_idx : (int)passes.size() - 1;
  for (size_t g = 0; g < pl.groups.size(); ++g) {
    const uint64_t gb = group_bits(pl.groups[g]);
    if ((int)g != main_g && (post_mask & gb))
      passes.push_back(PassSpec{(int)g, layer(ly.post, post_mask, pl.groups[g]), no_kick(),
                                dtc::kDiagNone, 0});
  }
  const double2* s2 = (const double2*)src;
  double2* d2 = (double2*)dst;
  const size_t len = (size_t)1 << nl;
  if (!dst) {
    // the chain's end: its one kick-only pass measures at its end, no store
    if (passes.size() != 1) return fail(DTC_EINVAL, "internal: measure-only end is one pass");
    DTC_TRY(launch_pass_spec(ctx, rc, 0, B, passes[0], s2, nullptr, dtc::kMeasSites, 1, n_obs,
                             meas_out, n_obs, nullptr, 0, 1));
    passes.clear();
  } else if (passes.empty()) {
    if (src != dst)
      DTC_HIP(hipMemcpyAsync(d2, s2, len * 16 * B, hipMemcpyDeviceToDevice, ctx->stream));
  }
  for (size_t i = 0; i < passes.size(); ++i) {
    const bool meas = obs && (int)i == meas_idx;
    DTC_TRY(launch_pass_spec(ctx, rc, 0, B, passes[i], i == 0 ? s2 : d2, d2,
                             meas ? dtc::kMeasSites : dtc::kMeasNone, diag ? 0 : 1, n_obs,
                             meas ? meas_out : nullptr, n_obs));
  }
  if (dst && obs && passes.empty()) {
    // no pass ran: measure with an identity-only kick pass over group 0
    PassSpec ps{0, layer(shard_forward_layer(1), 0, pl.groups[0]), no_kick(), dtc::kDiagNone, 0};
    ps.pre.row = 0;
    DTC_TRY(launch_pass_spec(ctx, rc, 0, B, ps, d2, d2, dtc::kMeasSites, 1, n_obs, meas_out,
                             n_obs));
  }
  if (obs_on_device) return DTC_OK;
  if (obs)
    DTC_HIP(hipMemcpyAsync(obs, ctx->vals_f.p, (size_t)B * n_obs * sizeof(double),
                           hipMemcpyDeviceToHost, ctx->stream));
  DTC_HIP(hipStreamSynchronize(ctx->stream));
  DTC_TRY(settle_pending(ctx));
  return DTC_OK;
}

// the echo twins' step: layers k and k + 1 of chain t around D*
int shard_echo_step_impl(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz,
                         const dtc_shard* sh, uint64_t seed, int64_t traj, int32_t inst,
                         int32_t t, int32_t k, uint64_t pre_mask, int32_t diag,
                         uint64_t post_mask, const double* src, double* dst, double* obs,
                         bool obs_on_device) {
  if (!ctx) return fail(DTC_EINVAL, "null ctx");
  DTC_TRY(shard_echo_check(pr, t, k));
  const int p = t + pr->t_offset;
  if (post_mask && k == p) return fail(DTC_EINVAL, "post_mask must be 0 at the chain's last layer");
  const ShardLayers ly{shard_echo_layer(t, p, k), shard_echo_layer(t, p, k + 1), dtc::kDiagConj};
  return shard_step_impl(ctx, pr, nz, sh, seed, traj, inst, ly, pre_mask, diag, post_mask, src,
                         dst, obs, obs_on_device, true);
}

int shard_kick_slice_impl(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz,
                          const dtc_shard* sh, uint64_t seed, int64_t traj, const ShardLayer& ly,
                          uint64_t pre_mask, int32_t chunk_bits, int32_t slice_bits,
                          int32_t slice, double* state) {
  if (!state) return fail(DTC_EINVAL, "null state");
  DTC_TRY(shard_check_common(ctx, pr, nz, sh, traj, 0));
  const int nl = sh->n_local;
  if (chunk_bits < 0 || slice_bits < 0 || chunk_bits + slice_bits > 16 ||
      nl - chunk_bits - slice_bits < dtc::kTileBits)
    return fail(DTC_EINVAL, "chunk_bits + slice_bits must leave >= 12 bits per slice");
  if (slice < 0 || slice >= (1 << slice_bits)) return fail(DTC_EINVAL, "slice out of range");
  const int nsub = nl - chunk_bits - slice_bits;
  const uint64_t low = (1ull << nsub) - 1;
  if (pre_mask & ~low) return fail(DTC_EINVAL, "slice kick mask reaches the chunk/slice bits");
  const int n_rows = std::max(1, pr->T - 1 + pr->t_offset);
  if (!pre_mask) return DTC_OK;
  if (ly.row < 0 || ly.row >= n_rows) return fail(DTC_EINVAL, "period outside kick table");
  const int64_t n_pieces = (int64_t)sh->n_shards << chunk_bits;
  if (n_pieces > 65535) return fail(DTC_EINVAL, "too many chunks x shards for one launch");
  DTC_HIP(hipSetDevice(ctx->device));
  RunCfg rc = shard_runcfg(pr, nz, sh, seed, traj);
  const Plan& pl = rc.pl;
  DTC_TRY(shard_kick_tables(ctx, pr, sh, rc));  // kick-only passes read no diagonal
  // one launch: the slice of every (shard, chunk) piece is a 2^nsub-amplitude
  // state, pieces 2^(nl - chunk_bits) apart (the same trajectory: identical
  // kick records for every piece)
  rc.L_eff_override = nsub;
  rc.stride_override = (int64_t)1 << (nl - chunk_bits);
  double2* base = (double2*)state + ((size_t)slice << nsub);
  for (size_t g = 0; g < pl.groups.size(); ++g) {
    const Group& G = pl.groups[g];
    const uint64_t gb = group_bits(G);
    if (!(pre_mask & gb)) continue;
    if (gb & ~low) return fail(DTC_EINVAL, "a site group of the kick mask reaches the slice bits");
    PassSpec ps{(int)g, no_kick(), no_kick(), dtc::kDiagNone, 0};
    ps.pre = shard_kick_desc(ly, G, pre_mask);
    DTC_TRY(launch_pass_spec(ctx, rc, 0, (int)n_pieces, ps, base, base, dtc::kMeasNone, 1, 2,
                             nullptr, 0));
  }
  return DTC_OK;
}

int shard_kick_exchange_slice_impl(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz,
                                   const dtc_shard* sh, uint64_t seed, int64_t traj,
                                   const ShardLayer& ly, uint64_t pre_mask, int32_t slice_bits,
                                   int32_t slice, double* state) {
  if (!ctx || !sh || !state) return fail(DTC_EINVAL, "null ctx/shard/state");
  const int k = sh->n_global, nl = sh->n_local;
  if (sh->n_shards != (1 << k) || sh->first_rank != 0)
    return fail(DTC_EINVAL, "the in-place exchange needs every shard in this buffer");
  DTC_TRY(shard_check_common(ctx, pr, nz, sh, traj, 0));
  if (slice_bits < 0 || k + slice_bits > 16 || nl - k - slice_bits < dtc::kTileBits)
    return fail(DTC_EINVAL, "chunk_bits + slice_bits must leave >= 12 bits per slice");
  if (slice < 0 || slice >= (1 << slice_bits)) return fail(DTC_EINVAL, "slice out of range");
  const int nsub = nl - k - slice_bits;
  const uint64_t low = (1ull << nsub) - 1;
  if (pre_mask & ~low) return fail(DTC_EINVAL, "slice kick mask reaches the chunk/slice bits");
  RunCfg rc = shard_runcfg(pr, nz, sh, seed, traj);
  const Plan& pl = rc.pl;
  const int n_rows = std::max(1, pr->T - 1 + pr->t_offset);
  if (ly.row < 0 || ly.row >= n_rows) return fail(DTC_EINVAL, "period outside kick table");
  // the group whose pass goes last carries the exchange (a unitary kick kind,
  // classified on the row that pass actually launches; launch_kick_swap takes
  // 1 <= k <= 6 chunk bits, other shapes run the two calls)
  int last = -1;
  for (size_t g = 0; g < pl.groups.size(); ++g)
    if (pre_mask & group_bits(pl.groups[g])) last = (int)g;
  bool fuse = last >= 0 && k >= 1 && k <= 6;
  if (fuse) {
    const Group& G = pl.groups[last];
    PassSpec ps{last, no_kick(), no_kick(), dtc::kDiagNone, 0};
    ps.pre = shard_kick_desc(ly, G, pre_mask);
    const int kind = pass_kind(rc, ps, dtc::kShapeK);
    fuse = kind == dtc::kKindRX || kind == dtc::kKindRY || kind == dtc::kKindGen;
  }
  if (!fuse) {
    DTC_TRY(shard_kick_slice_impl(ctx, pr, nz, sh, seed, traj, ly, pre_mask, k, slice_bits,
                                  slice, state));
    return dtc_shard_exchange_slice(ctx, sh, slice_bits, slice, state);
  }
  DTC_HIP(hipSetDevice(ctx->device));
  DTC_TRY(shard_kick_tables(ctx, pr, sh, rc));
  rc.L_eff_override = nsub;
  rc.stride_override = (int64_t)1 << (nl - k);
  double2* base = (double2*)state + ((size_t)slice << nsub);
  const int n_pieces = 1 << (2 * k);
  for (size_t g = 0; g < pl.groups.size(); ++g) {
    const Group& G = pl.groups[g];
    const uint64_t gb = group_bits(G);
    if (!(pre_mask & gb)) continue;
    if (gb & ~low) return fail(DTC_EINVAL, "a site group of the kick mask reaches the slice bits");
    PassSpec ps{(int)g, no_kick(), no_kick(), dtc::kDiagNone, 0};
    ps.pre = shard_kick_desc(ly, G, pre_mask);
    DTC_TRY(launch_pass_spec(ctx, rc, 0, n_pieces, ps, base, base, dtc::kMeasNone, 1, 2, nullptr,
                             0, nullptr, 0, 0, nullptr, (int)g == last ? k : 0));
  }
  return DTC_OK;
}

}  // namespace

extern "C" {

int dtc_shard_step(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz,
                   const dtc_shard* sh, uint64_t seed, int64_t traj, int32_t inst,
                   int32_t period, uint64_t pre_mask, int32_t diag, uint64_t post_mask,
                   const double* src, double* dst, double* obs) {
  return shard_step_impl(ctx, pr, nz, sh, seed, traj, inst, shard_forward_layers(period),
                         pre_mask, diag, post_mask, src, dst, obs, false);
}

int dtc_shard_step_async(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz,
                         const dtc_shard* sh, uint64_t seed, int64_t traj, int32_t inst,
                         int32_t period, uint64_t pre_mask, int32_t diag, uint64_t post_mask,
                         const double* src, double* dst, double* obs_dev) {
  return shard_step_impl(ctx, pr, nz, sh, seed, traj, inst, shard_forward_layers(period),
                         pre_mask, diag, post_mask, src, dst, obs_dev, true);
}

int dtc_shard_echo_step(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz,
                        const dtc_shard* sh, uint64_t seed, int64_t traj, int32_t inst,
                        int32_t t, int32_t k, uint64_t pre_mask, int32_t diag,
                        uint64_t post_mask, const double* src, double* dst, double* obs) {
  return shard_echo_step_impl(ctx, pr, nz, sh, seed, traj, inst, t, k, pre_mask, diag, post_mask,
                              src, dst, obs, false);
}

int dtc_shard_echo_step_async(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz,
                              const dtc_shard* sh, uint64_t seed, int64_t traj, int32_t inst,
                              int32_t t, int32_t k, uint64_t pre_mask, int32_t diag,
                              uint64_t post_mask, const double* src, double* dst,
                              double* obs_dev) {
  return shard_echo_step_impl(ctx, pr, nz, sh, seed, traj, inst, t, k, pre_mask, diag, post_mask,
                              src, dst, obs_dev, true);
}

int dtc_shard_kick_slice(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz,
                         const dtc_shard* sh, uint64_t seed, int64_t traj, int32_t period,
                         uint64_t pre_mask, int32_t chunk_bits, int32_t slice_bits, int32_t slice,
                         double* state) {
  return shard_kick_slice_impl(ctx, pr, nz, sh, seed, traj, shard_forward_layer(period), pre_mask,
                               chunk_bits, slice_bits, slice, state);
}

int dtc_shard_echo_kick_slice(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz,
                              const dtc_shard* sh, uint64_t seed, int64_t traj, int32_t t,
                              int32_t k, uint64_t pre_mask, int32_t chunk_bits,
                              int32_t slice_bits, int32_t slice, double* state) {
  if (!ctx) return fail(DTC_EINVAL, "null ctx");
  DTC_TRY(shard_echo_check(pr, t, k));
  return shard_kick_slice_impl(ctx, pr, nz, sh, seed, traj,
                               shard_echo_layer(t, t + pr->t_offset, k), pre_mask, chunk_bits,
                               slice_bits, slice, state);
}

int dtc_shard_kick_exchange_slice(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz,
                                  const dtc_shard* sh, uint64_t seed, int64_t traj,
                                  int32_t period, uint64_t pre_mask, int32_t slice_bits,
                                  int32_t slice, double* state) {
  return shard_kick_exchange_slice_impl(ctx, pr, nz, sh, seed, traj, shard_forward_layer(period),
                                        pre_mask, slice_bits, slice, state);
}

int dtc_shard_echo_kick_exchange_slice(dtc_ctx* ctx, const dtc_problem* pr, const dtc_noise* nz,
                                       const dtc_shard* sh, uint64_t seed, int64_t traj,
                                       int32_t t, int32_t k, uint64_t pre_mask,
                                       int32_t slice_bits, int32_t slice, double* state) {
  if (!ctx) return fail(DTC_EINVAL, "null ctx");
  DTC_TRY(shard_echo_check(pr, t, k));
  return shard_kick_exchange_slice_impl(ctx, pr, nz, sh, seed, traj,
                                        shard_echo_layer(t, t + pr->t_offset, k), pre_mask,
                                        slice_bits, slice, state);
}

int dtc_shard_exchange_slice(dtc_ctx* ctx, const dtc_shard* sh, int32_t slice_bits,
                             int32_t slice, double* state) {
  if (!ctx || !sh || !state) return fail(DTC_EINVAL, "null ctx/shard/state");
  const int nl = sh->n_local, k = sh->n_global;
  if (k < 1 || k > 6 || nl < 2 * k || nl > 40)
    return fail(DTC_EINVAL, "need 1 <= n_global <= 6 and n_local >= 2 n_global");
  if (sh->n_shards != (1 << k) || sh->first_rank != 0)
    return fail(DTC_EINVAL, "the in-place exchange needs every shard in this buffer");
  if (slice_bits < 0 || nl - k - slice_bits < dtc::kTileBits)
    return fail(DTC_EINVAL, "slice_bits must leave >= 12 bits per slice");
  if (slice < 0 || slice >= (1 << slice_bits)) return fail(DTC_EINVAL, "slice out of range");
  DTC_HIP(hipSetDevice(ctx->device));
  const int nsub = nl - k - slice_bits;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (ctx->prof) {
    e0 = get_event(ctx);
    e1 = get_event(ctx);
    DTC_HIP(hipEventRecord(e0, ctx->stream));
  }
  DTC_HIP(dtc::launch_exchange_swap((double2*)state, nl, k, nsub, slice, ctx->stream));
  if (ctx->prof) {
    DTC_HIP(hipEventRecord(e1, ctx->stream));
    // every off-diagonal piece read once and written once
    const double moved = (double)((1 << k) * ((1 << k) - 1)) * (double)((int64_t)1 << nsub);
    ctx->pending.push_back(Pending{DTC_KERNEL_EXCHANGE, e0, e1, 32.0 * moved});
  }
  return DTC_OK;
}

int dtc_get_stream(dtc_ctx* ctx, void** stream) {
  if (!ctx || !stream) return fail(DTC_EINVAL, "null ctx/stream");
  *stream = (void*)ctx->stream;
  return DTC_OK;
}

int dtc_synchronize(dtc_ctx* ctx) {
  if (!ctx) return fail(DTC_EINVAL, "null ctx");
  DTC_HIP(hipSetDevice(ctx->device));
  DTC_HIP(hipStreamSynchronize(ctx->stream));
  DTC_TRY(settle_pending(ctx));
  return DTC_OK;
}

}  // extern "C"
