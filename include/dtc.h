/*
 * dtc.h — C ABI of the MI355X DTC autocorrelator engine (libdtc_hip.so).
 *
 * This ABI replaces the one call the reference makes into its execution
 * engine for the DTC sweep:
 *
 *   backend = AerSimulator(noise_model=noise_model, device="GPU",
 *                          cuStateVec_enable=True)          fast.py:156
 *   backend.run(circ_tnoise, shots=1024).result()
 *          .get_counts(circ_tnoise)                          fast.py:211-212
 *   compute_z_expectation(counts, 1)[0]                      fast.py:92-109,213
 *
 * (fast.py = autocorr-delta-a-single-qiskit-fast.py; the same call appears at
 *  ...-polarization.py:219, ...-circular-polarization.py:241,
 *  ...-controlled-g.py:305, ...-g-optimization.py:309, ...-shots.py:214.)
 *
 * Aer runs one (L+1)-qubit circuit per time point t.  The engine instead runs
 * the folded L-qubit model: every time point of the
 * forward sweep comes from one trajectory, and every echo point t branches
 * off the forward state at t.  Results per trajectory are the ancilla
 * expectation value  a_r(t) = (1-p)^n_anc * z_j(init_r) * <Z_j>_r(t),
 * whose mean over trajectories is the expectation of
 * (n0 - n1)/shots in the reference.
 *
 * Conventions
 *  - Site i of the spin chain is bit i of the amplitude index (qiskit
 *    little-endian, circuit qubit i+1; the ancilla is folded away).
 *  - complex128 amplitudes, interleaved (re, im).
 *  - Kick matrices are complex 2x2, row-major, interleaved:
 *    {m00.re, m00.im, m01.re, m01.im, m10.re, m10.im, m11.re, m11.im}.
 *  - All host arrays are C-contiguous and owned by the caller.
 *  - Return value 0 = success; negative = error, message via
 *    dtc_last_error() (thread-local).  No C++ exception crosses the ABI.
 *  - Calls are synchronous (return after a stream sync).  One dtc_ctx per
 *    device per host thread; a ctx is not re-entrant.
 */
#ifndef DTC_H
#define DTC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DTC_ABI_VERSION 12

/* error codes */
#define DTC_OK 0
#define DTC_EINVAL (-1)   /* bad argument                          */
#define DTC_EHIP (-2)     /* HIP runtime error                     */
#define DTC_ENOMEM (-3)   /* device allocation failed              */
#define DTC_ENODEV (-4)   /* no usable gfx950 device               */

typedef struct dtc_ctx dtc_ctx;

/* One disorder sweep (fast.py:41-74 argparse + disorder load, and the circuit
 * family of fast.py:111-147 / ...-polarization.py:110-142 /
 * ...-controlled-g.py:196-241). */
typedef struct dtc_problem {
  int32_t L;           /* sites (fast.py --L)                              */
  int32_t T;           /* time points t = 0..T-1 (fast.py:48-51, --tf)      */
  int32_t n_inst;      /* disorder instances (fast.py --inst)              */
  int32_t probe_site;  /* j = int(L/2) (fast.py:221)                        */
  int32_t t_offset;    /* periods applied at t = t + t_offset: 0 for fast.py,
                          1 for controlled-g.py:416,467                    */
  int32_t n_sub;       /* noisy kick sub-gates per site per period:
                          1 (x, y), 2 (xy, yx, circular)                   */
  uint64_t init_mask;  /* Z-basis product state: bit i set = X on site i
                          (neel: fast.py:127-130)                          */
  const double* h;     /* [n_inst][L]   on-site RZ(h_i) angles              */
  const double* phi;   /* [n_inst][L-1] bond RZZ(phi_i) angles              */
  const double* kick;  /* [n_periods][L][n_sub][8] complex 2x2 kick gates,
                          row p = the (p+1)-th forward period,
                          n_periods = T - 1 + t_offset                     */
  int32_t want_fwd;    /* compute the forward autocorrelator              */
  int32_t want_echo;   /* compute the echo autocorrelator                 */
  int32_t batch;       /* states per device batch, 0 = automatic          */
  int32_t t_first;     /* outputs for t < t_first are skipped (left as 0):
                          a single-circuit call (one t) sets t_first = T-1 */
} dtc_problem;

/* Noise model (fast.py:76-86): depolarizing_error(p, 1) after every noisy
 * single-qubit gate (u2/u3 = kick gates, neel X prep, and n_anc ancilla
 * u2 gates).  p = 0 or use_noise = 0 means ideal. */
typedef struct dtc_noise {
  double p;
  int32_t n_anc;       /* noisy ancilla gates folded as (1-p)^n_anc: 6   */
  int32_t reserved;
} dtc_noise;

/* Device-like noise (the reference's
 * use_fakebackend=1 path, NoiseModel.from_backend(FakeBrisbane()) at
 * fast.py:77-79, whose calibration data is not available offline: the caller
 * supplies per-site calibration).  After every kick sub-gate on site i:
 *   thermal relaxation  amplitude damping gamma_i = 1 - exp(-gate_ns / T1_i)
 *                       and pure dephasing to the total coherence decay
 *                       exp(-gate_ns / T2_i)  (T2 clamped to 2 T1),
 *   then depolarizing_error(p_gate_i, 1).
 * Trajectories stay linear: the amplitude-damping Kraus operator is drawn with
 * fixed probabilities (jump w.p. gamma/2) and weighted by 1/sqrt(prob), so the
 * trajectory mean of the (unnormalized) <Z_j> is the exact channel's.  The
 * neel-prep X gates get the Pauli part only.  The ancilla enters as
 *   a = anc_factor * z_j(init) * <Z_j>,  reported as the read-out value
 *   (1 - p01 - p10) a + (p10 - p01)   (P(read 1|0) = p01, P(read 0|1) = p10). */
typedef struct dtc_device_noise {
  const double* p_gate;  /* [L] depolarizing parameter per kick sub-gate   */
  const double* t1_us;   /* [L] T1 (microseconds; <= 0 or inf: none)      */
  const double* t2_us;   /* [L] T2 (microseconds; <= 0 or inf: none)      */
  double gate_ns;        /* duration of one kick sub-gate                  */
  double anc_factor;     /* ancilla coherence factor ((1-p)^6 in fast.py)  */
  double readout_p01;    /* ancilla read-out P(1 | 0)                      */
  double readout_p10;    /* ancilla read-out P(0 | 1)                      */
} dtc_device_noise;

/* Context management. device = HIP device ordinal. */
int dtc_open(int32_t device, dtc_ctx** out);
int dtc_close(dtc_ctx* ctx);
/* Free the ctx's batch work buffers (state batches, partial sums, kick
 * records; the next call re-allocates what it needs) after waiting for its
 * stream -- e.g. before the caller allocates one 256 GiB sharded state on the
 * same device.  The forward prefix (dtc_prefix_*) is kept: call
 * dtc_prefix_release as well to free it (the Python wrapper does both). */
int dtc_release_buffers(dtc_ctx* ctx);
const char* dtc_last_error(void);
int32_t dtc_abi_version(void);

/* Full sweep for trajectories [traj_offset, traj_offset + n_traj) of every
 * instance.  Per-trajectory outputs (caller averages; see header comment):
 *   fwd   [n_inst][n_traj][T]     (nullable if !want_fwd)
 *   echo  [n_inst][n_traj][T]     (nullable if !want_echo)
 *   zsite [n_inst][n_traj][T][L]  forward per-site <Z_i>(t), nullable
 * Replaces the get_instances/get_single_out loops (fast.py:217-239) over
 * backend.run (fast.py:211).  The noise RNG is Philox4x32-10 keyed by seed
 * and counted by (global trajectory, stream, period, site, sub-gate), so
 * results do not depend on batching or on how trajectories are sharded. */
int dtc_autocorr(dtc_ctx* ctx, const dtc_problem* prob, const dtc_noise* noise,
                 uint64_t seed, int64_t traj_offset, int32_t n_traj,
                 double* fwd, double* echo, double* zsite);

/* dtc_autocorr under device-like noise (dtc_device_noise above); noise->p
 * and noise->n_anc are ignored.  Outputs as dtc_autocorr (zsite: unnormalized
 * per-site <Z_i>, nullable). */
int dtc_autocorr_device(dtc_ctx* ctx, const dtc_problem* prob, const dtc_device_noise* dev,
                        uint64_t seed, int64_t traj_offset, int32_t n_traj, double* fwd,
                        double* echo, double* zsite);

/* Two-qubit depolarizing noise on the chain's bonds: Aer's
 * depolarizing_error(p, 2), E(rho) = (1-p) rho + p I/4, after every RZZ of a
 * forward period and every RZZ^+ of an inverse period -- what a user writes as
 * noise_model.add_all_qubit_quantum_error(depolarizing_error(p2, 2), ["rzz"])
 * next to fast.py:84-86.  As a Pauli mixture: II with weight 1 - 15p/16, each
 * of the 15 other pairs p/16; p in [0, 16/15].  The ancilla is untouched (the
 * fold of SURVEY.md section 0.6 stays exact for a channel on the chain only).
 * Gate order as in the reference: forward period (fast.py:111-121) kicks, RZZ
 * on even bonds, RZZ on odd bonds, RZ; inverse period (fast.py:140-143) RZ^+,
 * RZZ^+ on odd bonds, RZZ^+ on even bonds, kick^+.
 * One Philox draw per (seed, trajectory, stream, counter, bond), (stream,
 * counter) those of the adjacent kick layer: forward period p (0, p), step k
 * of the echo at t (1 + t, k); disjoint from the kick draws, which stay
 * exactly as they are.  Rows do not depend on batching or sharding. */
typedef struct dtc_bond_noise {
  const double* p_bond;   /* [L-1], depolarizing_error(p, 2) parameter after the RZZ of bond b */
  int32_t reserved[2];
} dtc_bond_noise;

/* dtc_autocorr, or dtc_autocorr_device when dv != NULL (noise is ignored then, outputs
 * as dtc_autocorr_device: zsite unnormalised), with the channel above after every RZZ /
 * RZZ^+.  bond == NULL or every p_bond == 0: exactly dtc_autocorr / dtc_autocorr_device.
 * Under dv the forward runs K-D passes (dtc_schedule_counts[2]: nothing runs ahead, no
 * dual pass) and every echo chain keeps its trailing kick-only pass.  Relaxation during
 * the two-qubit gate is not modelled (the channel is the depolarizing one only).
 * DTC_EINVAL for p_bond outside [0, 16/15], prob->t_offset != 0, and a forward
 * prefix in place on the ctx (dtc_prefix_build; release it first).  Bond runs use the
 * plain chains (no light-cone end, no dual pass, DTC_SPLIT13 ignored); each diagonal
 * pass is preceded by one launch that builds its per-state factor tables (counted
 * under DTC_KERNEL_INIT when profiling). */
int dtc_autocorr_bond(dtc_ctx* ctx, const dtc_problem* prob, const dtc_noise* noise,
                      const dtc_device_noise* dv, const dtc_bond_noise* bond, uint64_t seed,
                      int64_t traj_offset, int32_t n_traj, double* fwd, double* echo,
                      double* zsite);

/* Host only, no device: the Pauli pairs drawn for one diagonal layer of one trajectory,
 * codes[b] = P_site_b + 4 * P_site_b+1 with 0 = I, 1 = X, 2 = Y, 3 = Z  (codes: [L-1]). */
int dtc_bond_draws(const dtc_bond_noise* bond, int32_t L, uint64_t seed, int64_t traj,
                   uint32_t stream, uint32_t counter, int32_t* codes);

/* Host only, no device, the twin of dtc_bond_draws for the kick gates: the Pauli code
 * (0 = I, 1 = X, 2 = Y, 3 = Z) drawn after every sub-gate of one kick layer of one
 * trajectory, pauli[site * n_sub + sub], with the thresholds of noise->p (dv == NULL) or
 * of dv (device-like noise: noise may be NULL); under dv, jump (nullable) receives the
 * amplitude-damping jump flag of each sub-gate (0 everywhere otherwise).  (stream,
 * counter): forward period p (0, p), step k of the echo at t (1 + t, k); (0xFFFFFFFF, 0)
 * gives the draws of the neel preparation's X gates (sub 0; Pauli only, no jump).  With
 * it a gate-by-gate model can follow a noisy trajectory through inverse periods. */
int dtc_kick_draws(const dtc_noise* noise, const dtc_device_noise* dv, int32_t L, int32_t n_sub,
                   uint64_t seed, int64_t traj, uint32_t stream, uint32_t counter,
                   int32_t* pauli, int32_t* jump);

/* Unit-test hook: apply n_periods Floquet periods to one host state vector
 * of 2^L complex128 amplitudes (in/out).  Forward: periods first_period,
 * first_period+1, ... (1-based rows of prob->kick), RNG stream `stream`,
 * RNG period counter = period.  Inverse (fast.py:140-143): periods
 * first_period, first_period-1, ..., each U_F^-1, RNG period counter =
 * step k = 1..n_periods.  zsite_out (nullable) receives [norm, <Z_0>..<Z_{L-1}>]
 * of the final state. */
int dtc_apply_periods(dtc_ctx* ctx, const dtc_problem* prob, const dtc_noise* noise,
                      uint64_t seed, int32_t inst, int64_t traj, uint32_t stream,
                      int32_t first_period, int32_t n_periods, int32_t inverse,
                      double* state, double* zsite_out);

/* ---- One state sharded over ranks (L=34 over 8 GPUs).
 * The 2^L amplitudes are split over 2^n_global ranks; a shard holds 2^n_local
 * amplitudes (n_local = L - n_global, 12 <= n_local <= 32).  Physical index bit
 * q < n_local of a shard holds logical site site_of[q]; bit k of the rank id
 * holds site site_of[n_local + k].  A call may hold n_shards consecutive ranks
 * (first_rank ..) whose shards lie 2^n_local amplitudes apart in one device
 * buffer ("virtual ranks": one GPU emulating several; 1 per process on a
 * multi-GPU node).  Every logical bond whose two sites are both local must join
 * physically adjacent bits.  The kick on a global site is applied after the
 * caller's all-to-all exchange has made it local (the sweep driver alternates
 * two bit maps, see sharded.py); the RZZ/RZ diagonal never needs one: bonds and
 * fields on rank bits become per-rank effective fields and a per-rank phase.
 * Replaces the reference's whole-state Aer run of a circuit too large for one
 * device; there is no reference call site for it (fast.py caps L at 20). */
typedef struct dtc_shard {
  int32_t n_local;
  int32_t n_global;
  int32_t n_shards;
  int32_t first_rank;
  int32_t site_of[64];
} dtc_shard;

/* state (device pointer, n_shards * 2^n_local complex128): the Z-basis product
 * state prob->init_mask of trajectory traj (noisy X preparation, fast.py:127-130,
 * drawn as in dtc_autocorr), distributed per site_of. */
int dtc_shard_set_basis(dtc_ctx* ctx, const dtc_problem* prob, const dtc_noise* noise,
                        const dtc_shard* shard, uint64_t seed, int64_t traj, double* state);

/* One step on every shard held (device pointers; src may equal dst):
 *   dst = K_{period+1}[post_mask] . D^diag . K_period[pre_mask] . src
 * where K_p[mask] = the period-p kick (fast.py:113, forward RNG stream 0, RNG
 * period counter p, trajectory traj) on the logical sites at the physical
 * local bits in mask, and D = the RZZ+RZ layer (fast.py:115-120) of instance
 * inst.  obs (host, nullable): [n_shards][1 + n_local] = (sum |a|^2,
 * sum z_q |a|^2 per physical bit q) of each shard after D (at the end when
 * diag = 0).  Synchronous. */
int dtc_shard_step(dtc_ctx* ctx, const dtc_problem* prob, const dtc_noise* noise,
                   const dtc_shard* shard, uint64_t seed, int64_t traj, int32_t inst,
                   int32_t period, uint64_t pre_mask, int32_t diag, uint64_t post_mask,
                   const double* src, double* dst, double* obs);

/* dtc_shard_step without waiting: everything is enqueued on the ctx's stream
 * (dtc_get_stream) and obs_dev (device pointer, nullable) receives
 * [n_shards][1 + n_local] from a device reduction.  The tables of a bit map are
 * built and uploaded on its first use and cached (a sweep alternates two), so
 * the host never blocks on the stream.  The sharded sweep driver orders its
 * exchanges against these steps with events (sharded.py), and reads obs_dev
 * after its own synchronisation. */
int dtc_shard_step_async(dtc_ctx* ctx, const dtc_problem* prob, const dtc_noise* noise,
                         const dtc_shard* shard, uint64_t seed, int64_t traj, int32_t inst,
                         int32_t period, uint64_t pre_mask, int32_t diag, uint64_t post_mask,
                         const double* src, double* dst, double* obs_dev);

/* The period-`period` kick on the local bits pre_mask, restricted to slice
 * `slice` of every chunk of every shard held: a shard's top chunk_bits local
 * bits number its chunks, the next slice_bits its slices, so the call covers the
 * amplitudes whose slice bits equal `slice` (in place; asynchronous, ctx stream;
 * one launch).  pre_mask must lie below the slice bits.  With chunk_bits =
 * n_global, chunk c is what rank c receives in the period's all-to-all; the
 * sweep driver kicks slice s+1 while slice s of every chunk travels to every
 * peer at once (sharded.py). */
int dtc_shard_kick_slice(dtc_ctx* ctx, const dtc_problem* prob, const dtc_noise* noise,
                         const dtc_shard* shard, uint64_t seed, int64_t traj, int32_t period,
                         uint64_t pre_mask, int32_t chunk_bits, int32_t slice_bits,
                         int32_t slice, double* state);

/* The last pre-exchange kicks of slice `slice` (as dtc_shard_kick_slice with
 * chunk_bits = n_global) fused with its in-place exchange (as
 * dtc_shard_exchange_slice): the pass of the last site group in pre_mask
 * stores piece (r, c) at (c, r), so the exchange moves no bytes of its own
 * (one GPU holding every shard; unitary kick kinds, else the two calls). */
int dtc_shard_kick_exchange_slice(dtc_ctx* ctx, const dtc_problem* prob, const dtc_noise* noise,
                                  const dtc_shard* shard, uint64_t seed, int64_t traj,
                                  int32_t period, uint64_t pre_mask, int32_t slice_bits,
                                  int32_t slice, double* state);

/* Virtual ranks only (one process holds every shard: n_shards = 2^n_global,
 * first_rank = 0): the period's all-to-all for slice `slice`, in place.  With
 * chunk bits = the top n_global local bits and slice bits = the next
 * slice_bits, piece (shard r, chunk c, slice) trades places with piece
 * (shard c, chunk r, slice) for every r != c -- what the 2^n_global ranks'
 * exchange of that slice does over xGMI, without a second state buffer (an
 * L=34 state, 256 GiB, then fits one MI355X).  Asynchronous, ctx stream, one
 * launch; 2^(n_local - n_global - slice_bits) >= 4096.  No reference call
 * site (the reference caps L at 20, fast.py:177-178). */
int dtc_shard_exchange_slice(dtc_ctx* ctx, const dtc_shard* shard, int32_t slice_bits,
                             int32_t slice, double* state);

/* ---- The echo on a sharded state (fast.py:140-143 on the layout above).
 * Chain t (p = t + prob->t_offset periods forward, F_p the state after them):
 *   E_t = K'_p ... D* K'_2 D* K'_1 D* F_p,  echo[t] ~ <Z_j>(E_t),
 * draw for draw dtc_autocorr's echo chain of that trajectory.  Layer k of
 * chain t, L_k:
 *   k = 0       the exact undo of the forward layer K_{p+1} (kick row p, forward
 *               stream 0, counter p + 1): the forward's fused step runs K_{p+1}
 *               ahead on its post_mask, and a chain forked there undoes it first
 *   1 <= k <= p K'_k, the inverse kick layer of period p - k + 1 (kick row
 *               p - k, sub-gates reversed and daggered, draws of RNG stream
 *               1 + t, counter k)
 * and D* is the conjugated RZZ+RZ layer (no communication, like D).  The four
 * calls below are their forward twins with (t, k) in place of `period`: the
 * same arguments otherwise, the same checks, plus 0 <= t < T, 0 <= k <= p and
 * every row used inside the kick table.
 *
 * dtc_shard_echo_step:  dst = L_{k+1}[post_mask] . (D*)^diag . L_k[pre_mask] . src
 * (post_mask must be 0 when k = p; src != dst forks a chain off the forward
 * buffer without a copy).  dst == NULL is a chain's end: with diag = 0,
 * post_mask = 0, a non-empty pre_mask inside one site group and obs given, one
 * kick-only pass measures obs at its end and stores nothing (16 B per
 * amplitude, DTC_KERNEL_FINAL_PASS); any other call with dst == NULL is
 * DTC_EINVAL.  An inverse period has the forward's shape mirrored: the fused
 * step after an exchange (pre = K'_k on the bits that just became local, D*,
 * post = K'_{k+1} on the top group), K'_{k+1} on the other local bits slice by
 * slice, the exchange (sharded.py: sharded_autocorr_pipelined). */
int dtc_shard_echo_step(dtc_ctx* ctx, const dtc_problem* prob, const dtc_noise* noise,
                        const dtc_shard* shard, uint64_t seed, int64_t traj, int32_t inst,
                        int32_t t, int32_t k, uint64_t pre_mask, int32_t diag,
                        uint64_t post_mask, const double* src, double* dst, double* obs);
int dtc_shard_echo_step_async(dtc_ctx* ctx, const dtc_problem* prob, const dtc_noise* noise,
                              const dtc_shard* shard, uint64_t seed, int64_t traj, int32_t inst,
                              int32_t t, int32_t k, uint64_t pre_mask, int32_t diag,
                              uint64_t post_mask, const double* src, double* dst,
                              double* obs_dev);
/* L_k of chain t on the local bits pre_mask of one slice (dtc_shard_kick_slice),
 * and the same fused with the slice's in-place exchange
 * (dtc_shard_kick_exchange_slice: unitary kick kinds, else the two calls). */
int dtc_shard_echo_kick_slice(dtc_ctx* ctx, const dtc_problem* prob, const dtc_noise* noise,
                              const dtc_shard* shard, uint64_t seed, int64_t traj, int32_t t,
                              int32_t k, uint64_t pre_mask, int32_t chunk_bits,
                              int32_t slice_bits, int32_t slice, double* state);
int dtc_shard_echo_kick_exchange_slice(dtc_ctx* ctx, const dtc_problem* prob,
                                       const dtc_noise* noise, const dtc_shard* shard,
                                       uint64_t seed, int64_t traj, int32_t t, int32_t k,
                                       uint64_t pre_mask, int32_t slice_bits, int32_t slice,
                                       double* state);

/* The ctx's HIP stream (hipStream_t), for ordering host-side collectives
 * against the asynchronous entry points; and a wait for everything on it. */
int dtc_get_stream(dtc_ctx* ctx, void** stream);
int dtc_synchronize(dtc_ctx* ctx);

/* Host-only: the site groups the engine's sharded steps use for an n_bits-bit
 * shard (high groups in increasing size: the top bits lie in a large group)
 * (bit masks, one per group; returns the count or a negative error). */
int32_t dtc_plan_groups(int32_t n_bits, uint64_t* masks, int32_t max_groups);

/* Forward prefix cache (the optimisation controller, SURVEY.md §8(f) row 2:
 * -g-optimization.py:359-427 re-runs the t+1-period circuit for every
 * candidate g of the last period; the t-period forward part is the same for
 * all candidates).
 * dtc_prefix_build: take the n_inst * n_traj trajectories (traj_offset ..)
 * of prob through periods 1..n_periods (noise keyed by seed, neel prep
 * included) and keep their states on the device, replacing any previous
 * prefix.  noise or dv (device-like noise, then noise is ignored).
 * dtc_autocorr_prefixed: dtc_autocorr (dv: dtc_autocorr_device, no zsite)
 * starting from those states: periods > n_periods and every echo draw their
 * noise from seed, the prefix periods keep theirs.  prob must match the
 * prefix's (instances, angles, kick rows 1..n_periods: checked by hash; the
 * same trajectories) and measure only after it (t_first + t_offset >
 * n_periods).  dtc_prefix_release frees the states. */
int dtc_prefix_build(dtc_ctx* ctx, const dtc_problem* prob, const dtc_noise* noise,
                     const dtc_device_noise* dv, uint64_t seed, int64_t traj_offset,
                     int32_t n_traj, int32_t n_periods);
int dtc_autocorr_prefixed(dtc_ctx* ctx, const dtc_problem* prob, const dtc_noise* noise,
                          const dtc_device_noise* dv, uint64_t seed, int64_t traj_offset,
                          int32_t n_traj, double* fwd, double* echo);
int dtc_prefix_release(dtc_ctx* ctx);

/* Energy observables of the forward sweep (the
 * BackendEstimatorV2 runs of autocorr-delta-a-single-qiskit-fast-energy*.py:
 * L-qubit circuit of fast.py's periods with no ancilla, energy.py:136-173).
 * Per trajectory and t (same schedule, noise and RNG contract as dtc_autocorr):
 *   z  [n_inst][n_traj][T][L]    <Z_i>
 *   zz [n_inst][n_traj][T][L-1]  <Z_i Z_{i+1}>      (nullable when L = 1)
 *   x  [n_inst][n_traj][T][L]    <X_i> (noiseless X-basis measurement)
 * in little-endian site order; the caller forms any Hamiltonian from them
 * (energy.py:83-102 builds its labels big-endian, see energy.py here). */
int dtc_energy(dtc_ctx* ctx, const dtc_problem* prob, const dtc_noise* noise, uint64_t seed,
               int64_t traj_offset, int32_t n_traj, double* z, double* zz, double* x);

/* dtc_energy under device-like noise (the FakeBrisbane estimator runs of
 * autocorr-delta-a-single-qiskit-fast-energy-fakebrisbane.py:131-192, with a
 * user-supplied calibration, see dtc_device_noise).  Same outputs, as the
 * Kraus-weighted (unnormalised) expectations of each trajectory: their mean is
 * the channel's expectation.  Read-out error is NOT applied here (anc_factor
 * and readout_p01/p10 are ignored); the caller maps the means (energy.py). */
int dtc_energy_device(dtc_ctx* ctx, const dtc_problem* prob, const dtc_device_noise* dv,
                      uint64_t seed, int64_t traj_offset, int32_t n_traj, double* z, double* zz,
                      double* x);

/* The energy estimator's trajectory means without the per-trajectory rows
 * (ABI 11): the same sweep as dtc_energy (dv == NULL) or dtc_energy_device
 * (dv != NULL; noise unused then), reduced over the n_traj trajectories of
 * each instance on the device:
 *   z_sum  [n_inst][T][L], zz_sum [n_inst][T][L-1] (nullable when L = 1),
 *   x_sum  [n_inst][T][L]
 * = the sums over trajectories of dtc_energy's z, zz, x (fixed summation
 * order within a batch, batches added on the host: equal to the host sums of
 * those rows, and invariant under a change of batch size, only up to
 * rounding -- unlike the per-trajectory rows, which are bit-identical for any
 * batching).  The energy
 * scripts need only these means (energy.py:136-173: <H> from the estimator's
 * expectation values); only a few KB per batch cross PCIe. */
int dtc_energy_sums(dtc_ctx* ctx, const dtc_problem* prob, const dtc_noise* noise,
                    const dtc_device_noise* dv, uint64_t seed, int64_t traj_offset,
                    int32_t n_traj, double* z_sum, double* zz_sum, double* x_sum);

/* dtc_energy / dtc_energy_device (dv != NULL; noise ignored then) and
 * dtc_energy_sums with dtc_bond_noise's channel after every RZZ.  The energy
 * circuit has forward layers only: the draws of forward period p are (stream 0,
 * counter p), p = t + t_offset (any t_offset, as in dtc_energy).  bond == NULL
 * or every p_bond == 0: exactly the plain entry points.  The observables of
 * time t are taken on the state before the layer's outgoing Pauli P_t (which
 * the next kick layer absorbs): one launch per batch then negates <Z_i> where
 * P_t has X content on i, <Z_i Z_i+1> by the product of its two sites' flips
 * and <X_i> where P_t has Z content, on the device, before the rows are read
 * back or summed (counted under DTC_KERNEL_REDUCE when profiling). */
int dtc_energy_bond(dtc_ctx* ctx, const dtc_problem* prob, const dtc_noise* noise,
                    const dtc_device_noise* dv, const dtc_bond_noise* bond, uint64_t seed,
                    int64_t traj_offset, int32_t n_traj, double* z, double* zz, double* x);
int dtc_energy_sums_bond(dtc_ctx* ctx, const dtc_problem* prob, const dtc_noise* noise,
                         const dtc_device_noise* dv, const dtc_bond_noise* bond, uint64_t seed,
                         int64_t traj_offset, int32_t n_traj, double* z_sum, double* zz_sum,
                         double* x_sum);

/* The energy echo (additive, ABI 12 unchanged): the energy observables of the
 * Loschmidt echo, the circuit qc_qiskit(..., echo=True) of the energy scripts
 * builds (...-fast-energy.py:141-153: t forward periods, then
 * UF_subcircuit.inverse() t times) and hands to the estimator.  Outputs as
 * dtc_energy / dtc_energy_sums; row t holds <Z_i>, <Z_i Z_i+1>, <X_i> of the
 * state E_t = the forward state after p = t + t_offset periods taken through p
 * inverse periods -- the state dtc_autocorr measures its echo on, drawn the
 * same way: forward period q (stream 0, counter q), step k of the echo at t
 * (stream 1 + t, counter k; it undoes period p - k + 1), the neel preparation
 * as in dtc_energy.  So z[..][t][probe_site] is what dtc_autocorr's echo[..][t]
 * is made from.  Without noise every row equals the initial state's.
 * Row p = 0 is formed from the initial mask on the host; prob->t_first is
 * honoured as in dtc_autocorr (chains for t < t_first are not built, their
 * rows are 0); want_fwd / want_echo are ignored and the forward is not
 * measured (dtc_energy gives the forward energy).  Rows are bit-identical
 * under any batching and any split of the trajectories; the sums are reduced
 * on the device as dtc_energy_sums' and are batch-invariant up to rounding.
 * The schedule is dtc_autocorr's echo sweep (dual pass, wavefront interior)
 * without the light-cone end and with every chain's trailing kick-only pass
 * kept: the pass applying a site group's last kicks measures X of that group
 * after them, the chain's last pass norm, Z, ZZ of all sites, and stores
 * nothing (DTC_KERNEL_FINAL_PASS).  Depolarizing or noiseless kicks of every
 * family dtc_energy takes; device-like noise and bond noise are not covered
 * (there is no entry point taking them: the Python wrapper refuses). */
int dtc_energy_echo(dtc_ctx* ctx, const dtc_problem* prob, const dtc_noise* noise, uint64_t seed,
                    int64_t traj_offset, int32_t n_traj, double* z, double* zz, double* x);
int dtc_energy_echo_sums(dtc_ctx* ctx, const dtc_problem* prob, const dtc_noise* noise,
                         uint64_t seed, int64_t traj_offset, int32_t n_traj, double* z_sum,
                         double* zz_sum, double* x_sum);

/* Measurement sampling (additive, ABI 12 unchanged): what a measurement of the
 * chain itself returns, a bitstring -- the counts BackendEstimatorV2 forms its
 * expectation values from (...-fast-energy.py:168-171: 4096 shots per commuting
 * group, the Z-type and the X-type terms of H each in their own basis).  For
 * every trajectory of dtc_energy and every time t, n_shots outcomes in the Z
 * basis and n_shots in the X basis of the forward state after p = t + t_offset
 * periods.
 *
 * A sample: for the state psi (2^L amplitudes, site i = bit i) let
 * S(x) = sum_{y <= x} |psi_y|^2 in ascending index order and W = S(2^L - 1)
 * (1 up to rounding).  For a uniform u in [0, 1) the Z-basis outcome is the
 * smallest x with S(x) > u W; the X-basis outcome is the same rule on
 * H^(x)L psi (a noiseless basis change, as dtc_energy measures X): bit i set
 * means X_i = -1.  An index of zero weight is never returned.
 *
 * The uniforms: Philox4x32-10 with the key of the kick draws and the counter
 *   c0 = shot | basis << 30   (basis 0 = Z, 1 = X; shot < 2^30),
 *   c1 = p, c2 = 0xFFFFFFFE (the measurement stream), c3 = (uint32_t)traj,
 *   u = (((uint64_t)w0 << 21) | (w1 >> 11)) * 2^-53.
 * No kick, preparation or bond draw has c2 = 0xFFFFFFFE, and the kick draws stay
 * exactly as they are: a sampled run's trajectories are dtc_energy's, trajectory
 * for trajectory.  Row p = 0 follows the rule on the prepared basis state: Z
 * gives the (noisily) prepared mask, X gives floor(u 2^L).
 *
 * Rows are bit-identical for any batch size, any split of the trajectories and
 * either batch layout: the sums behind S are formed in a fixed hierarchy over
 * the logical index (dtc_sample.hip), which agrees with the sequential S of
 * dtc_sample_state up to rounding of the sums (an outcome may differ only
 * where u W lies within that rounding of a boundary S(x)).
 *
 * The forward runs in K-D passes (after the pass closing period p the state at
 * p is in memory exactly, nothing runs a kick layer ahead); each sampled state
 * costs one extra read per basis (the weights; the picks read one 64 KiB chunk
 * per shot), the X basis one basis-change pass per site group before it.
 * Launches are counted under DTC_KERNEL_REDUCE when profiling.  Depolarizing or
 * noiseless kicks only: under device-like noise a shot would have to be
 * weighted by the Kraus norm, and bond noise has no sampled entry point either
 * (the Python wrapper refuses both).  The echo state is never stored, so it is
 * not sampled.
 *
 * zbits, xbits: [n_inst][n_traj][T][n_shots] uint64, either may be NULL (not both);
 * rows t < prob->t_first are left 0; want_fwd / want_echo ignored.
 * DTC_EINVAL for null arguments, n_shots < 1 and L > 32. */
int dtc_sample(dtc_ctx* ctx, const dtc_problem* prob, const dtc_noise* noise, uint64_t seed,
               int64_t traj_offset, int32_t n_traj, int32_t n_shots, uint64_t* zbits,
               uint64_t* xbits);
/* host only: the uniforms of (seed, traj, p, basis), u[n_shots] */
int dtc_sample_draws(uint64_t seed, int64_t traj, int32_t p, int32_t basis, int32_t n_shots,
                     double* u);
/* host only, the contract's reference: outcomes of n uniforms on a host state of 2^L
 * complex128 amplitudes (sequential S in index order); basis 1 applies H^L first. */
int dtc_sample_state(const double* state, int32_t L, int32_t basis, const double* u, int32_t n,
                     uint64_t* bits);

/* All-pair correlators of the forward sweep (no reference counterpart: the
 * reference measures the nearest-neighbour terms of H only).  For every
 * trajectory of dtc_energy and every time t, on the forward state psi after
 * p = t + t_offset periods (2^L amplitudes, site i = bit i, z_i(y) = +1 / -1 for
 * bit i of y clear / set):
 *   z[i]          = sum_y |psi_y|^2 z_i(y)                  <Z_i>
 *   zz[(i, j)]    = sum_y |psi_y|^2 z_i(y) z_j(y), i < j    <Z_i Z_j>
 * and x, xx: the same sums on H^(x)L psi, <X_i> and <X_i X_j> (a noiseless
 * basis change, as dtc_energy measures X).  Pairs are in row-major order (0,1),
 * (0,2), ..., (L-2,L-1): pair (i, j) is entry i (2L - i - 1) / 2 + j - i - 1.
 * The sums are not divided by the norm (1 up to rounding: depolarizing or
 * noiseless kicks only; the Python wrapper refuses device-like and bond noise).
 * Every sum is linear in |psi><psi|, so the mean over trajectories estimates the
 * depolarizing channel's exact expectation; the
 * trajectories are dtc_energy's, trajectory for trajectory (no new draws):
 * zz[(i, i+1)], z and x are dtc_energy's values up to rounding.
 *
 * Row p = 0 is formed on the host from the prepared mask m: z[i] = z_i(m),
 * zz[(i, j)] = z_i(m) z_j(m), x = xx = 0.
 *
 * Rows are bit-identical for any batch size, any split of the trajectories and
 * either batch layout: every sum is formed in a fixed hierarchy over the
 * logical index (dtc_corr.hip; DESIGN.md "All-pair correlators").
 *
 * The forward runs in dtc_sample's K-D passes; each measured state costs one
 * extra read per basis (and a small reduce over the chunk partials), the X
 * basis one basis-change pass per site group before it.  Launches are counted
 * under DTC_KERNEL_REDUCE when profiling, the read with 16 B per amplitude.
 *
 * z, x: [n_inst][n_traj][T][L]; zz, xx: [n_inst][n_traj][T][L (L - 1) / 2]; any may
 * be NULL (not all): the Z launches run iff z or zz is given, the X-basis
 * passes and launches iff x or xx is.  Rows t < prob->t_first are left 0;
 * want_fwd / want_echo ignored.  DTC_EINVAL for a null ctx, all outputs null
 * and L > 32. */
int dtc_correlations(dtc_ctx* ctx, const dtc_problem* prob, const dtc_noise* noise, uint64_t seed,
                     int64_t traj_offset, int32_t n_traj, double* z, double* zz, double* x,
                     double* xx);
/* The same sweep with the per-trajectory rows summed per instance on the device:
 * z_sum, x_sum [n_inst][T][L], zz_sum, xx_sum [n_inst][T][L (L - 1) / 2] (divide by
 * n_traj for the means).  Batch-invariant up to rounding only: an instance's
 * trajectories are added batch by batch. */
int dtc_correlation_sums(dtc_ctx* ctx, const dtc_problem* prob, const dtc_noise* noise,
                         uint64_t seed, int64_t traj_offset, int32_t n_traj, double* z_sum,
                         double* zz_sum, double* x_sum, double* xx_sum);
/* host only, the contract's reference: z [L] and zz [L (L - 1) / 2] of a host state of
 * 2^L complex128 amplitudes; basis 1 applies H^L first.  The chunk partials by
 * plain loops, combined with the kernels' own index algebra (csrc/dtc_corr.h). */
int dtc_correlations_state(const double* state, int32_t L, int32_t basis, double* z, double* zz);

/* Reduced density matrices of site windows of the forward sweep (no reference
 * counterpart).  A window is k sites s_0 < s_1 < ... < s_{k-1}, 1 <= k <= 4; all
 * n_win windows of a call share k (sites: [n_win][k]).  With d = 2^k, row index
 * alpha has bit m equal to the bit of site s_m, and for every trajectory of
 * dtc_energy and every time t, on the forward state psi after p = t + t_offset
 * periods,
 *   rho[alpha][alpha'] = sum_c psi(alpha, c) conj psi(alpha', c),
 * c running over the other L - k bits: rho = Tr_rest |psi><psi|.  In this
 * convention <O_{s_1} (x) O_{s_0}> = Tr(rho kron(O_{s_1}, O_{s_0})) (the last
 * site is the most significant factor), e.g. <Z_{s_0}> = rho[0][0] - rho[1][1]
 * for k = 1.  rho is not divided by the norm (Tr rho = 1 up to rounding:
 * depolarizing or noiseless kicks only; the Python wrapper refuses device-like
 * and bond noise).  The stored matrix is Hermitian bit for bit -- one triangle
 * is computed, the other is its conjugate -- and the imaginary part of the
 * diagonal is exactly 0.
 *
 * rho is linear in |psi><psi|, so the mean over trajectories estimates the
 * depolarizing channel's exact reduced state; quantities
 * that are not linear in rho (entropy, purity, mutual information) must be
 * taken of that mean, not averaged per trajectory.  The trajectories are
 * dtc_energy's, trajectory for trajectory (no new draws), reached through the
 * K-D schedule of dtc_sample and dtc_correlations.
 *
 * Row p = 0 is formed on the host from the prepared mask m: rho = |m_A><m_A|,
 * the single entry 1 at alpha = alpha' = the bits of m at the window's sites.
 * Rows t < prob->t_first are left 0; want_fwd / want_echo ignored.
 *
 * Rows are bit-identical for any batch size, any split of the trajectories and
 * either batch layout: every sum is a fixed function of the logical index, and
 * no atomics are used (dtc_rdm.hip; DESIGN.md "Reduced density matrices").
 *
 * Each measured state costs one extra read per window (and a small reduce over
 * the workgroup partials); no basis-change pass.  Launches are counted under
 * DTC_KERNEL_REDUCE when profiling, the read with 16 B per amplitude.
 *
 * rho: [n_inst][n_traj][T][n_win][d][d][2] (re, im).  DTC_EINVAL for null
 * arguments, n_win < 1, k outside 1..4, k > L, a site outside [0, L), sites of
 * a window not strictly ascending, L > 32, and T n_win d d > 2^25. */
int dtc_rdm(dtc_ctx* ctx, const dtc_problem* prob, const dtc_noise* noise, uint64_t seed,
            int64_t traj_offset, int32_t n_traj, const int32_t* sites, int32_t n_win, int32_t k,
            double* rho);
/* The same sweep with the per-trajectory matrices summed per instance on the
 * device: rho_sum [n_inst][T][n_win][d][d][2] (divide by n_traj for the mean
 * state).  Batch-invariant up to rounding only: an instance's trajectories are
 * added batch by batch. */
int dtc_rdm_sums(dtc_ctx* ctx, const dtc_problem* prob, const dtc_noise* noise, uint64_t seed,
                 int64_t traj_offset, int32_t n_traj, const int32_t* sites, int32_t n_win,
                 int32_t k, double* rho_sum);
/* host only, the contract's reference: rho [d][d][2] of one window of a host
 * state of 2^L complex128 amplitudes, by plain sums over c in ascending order
 * with the kernels' own index algebra (csrc/dtc_rdm.h).  The same checks as
 * dtc_rdm, without a device. */
int dtc_rdm_state(const double* state, int32_t L, const int32_t* sites, int32_t k, double* rho);

/* Reduced density matrices of blocks of contiguous sites of the forward sweep
 * (no reference counterpart): the half-chain entanglement.  A block is the k
 * sites a, a+1, ..., a+k-1, given as its start a; all n_blk blocks of a call
 * share k, 5 <= k <= 10 (k <= 4: dtc_rdm).  Index convention of dtc_rdm: with
 * d = 2^k, bit m of a row index is the bit of site a + m, and
 *   rho[alpha][alpha'] = sum_c psi(alpha, c) conj psi(alpha', c)
 * on the forward state psi after p = t + t_offset periods.  The sweep, the
 * trajectories and the draws are dtc_rdm's (the K-D schedule of dtc_sample; no
 * new draws).  Depolarizing or noiseless kicks only; the Python wrapper refuses
 * device-like and bond noise.
 *
 * rho_sum [n_inst][T][n_blk][d][d][2] (nullable): the sum over an instance's
 * trajectories of the per-state rho; nothing is divided by the norm or by
 * n_traj.  Hermitian bit for bit -- one triangle is computed, the other is its
 * conjugate -- with the diagonal's imaginary part exactly 0.  Batch-invariant up
 * to rounding only, like dtc_rdm_sums.  Linear in |psi><psi|: the trajectory
 * mean is the depolarizing channel's exact reduced state.
 *
 * purity [n_inst][n_traj][T][n_blk] (nullable; not both null):
 * sum_{alpha alpha'} |rho[alpha][alpha']|^2 of that trajectory's own (pure)
 * state: -ln of it is the trajectory-resolved second Renyi entanglement
 * entropy.  Summed in an order that is a function of the logical index alone:
 * rows are bit-identical for any batch size, any split of the trajectories and
 * either batch layout.  No atomics anywhere.
 *
 * Row p = 0 is formed on the host from the prepared mask m: rho = |m_A><m_A|,
 * purity 1.  Rows t < prob->t_first are left 0; want_fwd / want_echo ignored.
 *
 * Cost per measured state and block: about 2^(L+k+2) FP64 flops (the lower
 * triangle, FP64 MFMA) against the state's 16 B per amplitude; compute-bound
 * beyond k = 5..6 (DESIGN.md "Block density matrices").  Launches are counted
 * under DTC_KERNEL_REDUCE when profiling.
 *
 * DTC_EINVAL, before any device call, for null arguments, n_blk < 1, k outside
 * 5..10, 2 k > L, start < 0, start + k > L, L > 32 and T n_blk d d > 2^25. */
int dtc_rdm_block_sums(dtc_ctx* ctx, const dtc_problem* prob, const dtc_noise* noise,
                       uint64_t seed, int64_t traj_offset, int32_t n_traj, const int32_t* starts,
                       int32_t n_blk, int32_t k, double* rho_sum, double* purity);
/* host only, the contract's reference: rho [d][d][2] (nullable) and purity [1]
 * of one block of a host state of 2^L complex128 amplitudes, by plain loops over
 * the column index in ascending order with the kernels' own index algebra
 * (csrc/dtc_rdm_block.h).  The same block checks, without a device.  Agrees with
 * the device to rounding, not to bits. */
int dtc_rdm_block_state(const double* state, int32_t L, int32_t start, int32_t k, double* rho,
                        double* purity);

/* Profiling: when enabled, every kernel launch is bracketed by HIP events on
 * the ctx stream and accumulated per kernel kind. */
#define DTC_KERNEL_LO_PASS 0   /* fused RZZ+RZ diagonal + low-site kick pass */
#define DTC_KERNEL_HI_PASS 1   /* high-site kick pass                        */
#define DTC_KERNEL_REDUCE 2    /* per-state observable reduction; bond-noise sign pass;
                                  measurement sampling (weights, picks); all-pair
                                  correlators (chunk partials, their reduce) */
#define DTC_KERNEL_INIT 3      /* preparation: bond-noise diagonal table builder */
#define DTC_KERNEL_FINAL_PASS 4 /* last pass of an echo chain (sharded ones too): measure, no store */
#define DTC_KERNEL_EXCHANGE 5  /* virtual ranks' in-place slice exchange        */
#define DTC_KERNEL_KINDS 6
/* total_bytes = algorithmic HBM bytes of the launches: 32 B per amplitude for a
 * pass that reads and stores its state, 16 B for one that only reads
 * (measure-only) or only stores (the first pass of a sweep, which forms the
 * basis states in registers), 32 B per amplitude an exchange moves. */
int dtc_set_profiling(dtc_ctx* ctx, int32_t on);
int dtc_kernel_stats(dtc_ctx* ctx, int32_t kind, int64_t* launches,
                     double* total_ms, double* total_bytes);
int dtc_reset_stats(dtc_ctx* ctx);
/* Light-cone ends launched since dtc_open, by kernel: counts[0] the 8-site
 * window (dtc_lc_final*), [1] the 10-site window's generic kernel
 * (dtc_lcw_final), [2] its three-re-layout C2 form (dtc_lcw2_final), [3] the
 * 12-site window (dtc_lcw3_final, six passes merged; ABI 10).
 * Independent of profiling; lets tests assert which kernel a sweep ran. */
int dtc_lightcone_counts(dtc_ctx* ctx, int64_t* counts /* [4] */);
/* Batch schedules built since dtc_open (ABI 12; test hook, no reference
 * counterpart): counts[0] echo chains whose first pass folded into the
 * forward's dual pass, [1] device-noise batches whose forward ran one kick
 * layer ahead (one pass per period), [2] device-noise batches run with K-D
 * forward passes (a chain did not fold, or DTC_NO_RUNAHEAD=1, the test switch
 * that forces this schedule; two passes per period), [3] batches run with the
 * 13 / 7 site split of L = 20 (a 13-site group in 8192-amplitude tiles, a
 * 7-site column group; opt-in with DTC_SPLIT13=1, the default keeps the
 * 12 / 8 split). */
int dtc_schedule_counts(dtc_ctx* ctx, int64_t* counts /* [4] */);

/* Wavefront passes launched since the engine opened: stored passes that advance
 * an echo chain's interior by several kick layers per read and write of the
 * state, over two tiles that share site 11 (L = 20, the 12 / 8 plan, unitary
 * RX / RY kicks, depolarizing noise only, the octet layout; DESIGN.md section
 * 4).  On by default; an engine opened with DTC_NO_WAVEFRONT=1 in the
 * environment keeps the plain interior (the test switch), DTC_WAVEFRONT=2..4
 * sets the layer cap per pass (default 4; a plan must take fewer launches than
 * the plain interior, except at cap 2, which cannot and runs its two-step passes
 * at the plain count: a test switch).  Booked under DTC_KERNEL_LO_PASS. */
int dtc_wavefront_count(dtc_ctx* ctx, int64_t* count);

/* Device properties for reports. */
int dtc_device_info(dtc_ctx* ctx, char* name, int32_t name_len, int32_t* n_cu,
                    double* hbm_bytes);

#ifdef __cplusplus
}
#endif
#endif /* DTC_H */
