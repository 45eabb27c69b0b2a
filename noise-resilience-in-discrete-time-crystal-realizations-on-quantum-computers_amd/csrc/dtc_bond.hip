// dtc_bond.hip — two-qubit depolarizing noise on the RZZ bonds: the per-state
// diagonal factor tables of one diagonal layer (dtc_kernels.h BondDiagArgs), and
// the signs of the outgoing Paulis on the energy observables (BondObsArgs).
//
// The channel after every RZZ / RZZ^+ is a Pauli mixture (dtc_rng.h
// sample_bond).  A Pauli pushed through the rest of the diagonal layer only
// flips the sign of the angles it anticommutes with, so a trajectory's noisy
// layer is the same diagonal with some angles negated, followed by a layer of
// single-site Paulis that the next kick layer absorbs (dtc_kernels.hip
// build_site_kick).  With xL_b / xR_b = the error of bond b has X or Y on
// site b / site b+1 (0 for a missing bond):
//   forward layer (RZZ even, RZZ odd, RZ):  odd bond b   (-1)^(xR_{b-1} + xL_{b+1})
//                                           field i      (-1)^(xR_{i-1} + xL_i)
//   inverse layer (RZ^+, RZZ^+ odd, even):  even bond b  (-1)^(xR_{b-1} + xL_{b+1})
// The pass kernels index the tables by state when they are launched with
// batch_start = 0, n_traj = 1 (PassArgs): no change in them.
//
// One workgroup per state: the layer's L-1 pairs are drawn once into LDS, the
// flip masks formed, then the (n_chunks + L_eff) * 64 entries filled with f64
// sincos -- 24.5 KB per state at L = 20 against a 16 MB state.
#include <hip/hip_runtime.h>

#include "dtc_kernels.h"
#include "dtc_rng.h"

namespace dtc {

namespace {

// The angle of build_diag_tables' diag_angle with the layer's signs: fields of
// sites [lo_site, hi_site), bonds [bond_lo, bond_hi), z_i from bit i - bit0 of v.
__device__ __forceinline__ double signed_angle(int L, const double* hh, const double* pp,
                                               uint32_t fflip, uint32_t bflip, int lo_site,
                                               int hi_site, int bond_lo, int bond_hi, int bit0,
                                               int v) {
  double ang = 0.0;
  for (int i = lo_site; i < hi_site && i < L; ++i) {
    const bool neg = (((v >> (i - bit0)) & 1) ^ ((fflip >> i) & 1u)) != 0;
    ang += neg ? -hh[i] : hh[i];
  }
  for (int i = bond_lo < 0 ? 0 : bond_lo; i < bond_hi && i + 1 < L; ++i) {
    const bool neg =
        (((v >> (i - bit0)) & 1) ^ ((v >> (i + 1 - bit0)) & 1) ^ ((bflip >> i) & 1u)) != 0;
    ang += neg ? -pp[i] : pp[i];
  }
  return ang;
}

__global__ __launch_bounds__(256) void bond_diag_kernel(BondDiagArgs A) {
  __shared__ uint32_t s_x[2];     // bit b: xL_b, xR_b
  __shared__ uint32_t s_flip[2];  // field / bond sign flips
  const int b = blockIdx.x;
  if (b >= A.batch) return;
  const int64_t gstate = A.batch_start + b;
  const int inst = (int)(gstate / A.n_traj);
  const uint64_t traj = (uint64_t)(A.traj_offset + gstate % A.n_traj);
  const int L = A.L;
  if (threadIdx.x < 2) s_x[threadIdx.x] = 0u;
  __syncthreads();
  if ((int)threadIdx.x < L - 1) {
    const int bond = (int)threadIdx.x;
    const int code = sample_bond(A.seed, traj, A.stream, A.counter, (uint32_t)bond, A.thr[bond]);
    if (pauli_has_x(code & 3)) atomicOr(&s_x[0], 1u << bond);
    if (pauli_has_x(code >> 2)) atomicOr(&s_x[1], 1u << bond);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t xl = s_x[0], xr = s_x[1];
    // site i sees xR_{i-1} and xL_i; bond b sees xR_{b-1} and xL_{b+1}
    const uint32_t site_x = (xr << 1) ^ xl;
    const uint32_t bond_x = (xr << 1) ^ (xl >> 1);
    const uint32_t odd = 0xAAAAAAAAu;
    s_flip[0] = A.inverse ? 0u : site_x;
    s_flip[1] = bond_x & (A.inverse ? ~odd : odd);
  }
  __syncthreads();
  const uint32_t fflip = s_flip[0], bflip = s_flip[1];
  const double* hh = A.h + (int64_t)inst * L;
  const double* pp = A.phi + (int64_t)inst * (L > 1 ? L - 1 : 0);
  double2* o = A.out + (int64_t)b * A.diag_stride;
  for (int e = (int)threadIdx.x; e < A.diag_stride; e += 256) {
    const int k = e >> 6, v = e & 63;
    double ang;
    if (k < A.n_chunks) {
      const int b0 = kChunkBits * k;
      ang = signed_angle(L, hh, pp, fflip, bflip, b0, b0 + kChunkBits, b0, b0 + kChunkBits, b0, v);
    } else {
      const int g0 = k - A.n_chunks;
      if (g0 == 0 && (v & 1)) {  // bit -1 does not exist
        o[e] = make_double2(0.0, 0.0);
        continue;
      }
      ang = signed_angle(L, hh, pp, fflip, bflip, g0, g0 + 4, g0 - 1, g0 + 4, g0 - 1, v);
    }
    double sn, cs;
    sincos(-0.5 * ang, &sn, &cs);
    o[e] = make_double2(cs, sn);
  }
}

// The signs that the outgoing Pauli P_t of forward layer t + t_offset leaves on
// the energy observables of time t (dtc_kernels.h BondObsArgs).  One workgroup
// (one wave) per (state, t): the layer's L-1 pairs are drawn once into LDS as
// four masks (X / Z content of the left and right parts), merged per site, and
// the row's 3 L - 1 entries after the norm negated where the rule says so --
// a few hundred bytes per row, no state traffic.
__global__ __launch_bounds__(64) void bond_obs_sign_kernel(BondObsArgs A) {
  __shared__ uint32_t s_m[4];  // xL, xR, zL, zR (bit b: bond b)
  const int t = (int)(blockIdx.x % (unsigned)A.T);
  const int b = (int)(blockIdx.x / (unsigned)A.T);
  if (b >= A.batch || t + A.t_offset == 0) return;  // uniform per workgroup
  const int64_t gstate = A.batch_start + b;
  const uint64_t traj = (uint64_t)(A.traj_offset + gstate % A.n_traj);
  const int L = A.L;
  if (threadIdx.x < 4) s_m[threadIdx.x] = 0u;
  __syncthreads();
  if ((int)threadIdx.x < L - 1) {
    const int bond = (int)threadIdx.x;
    const int code = sample_bond(A.seed, traj, kStreamForward, (uint32_t)(t + A.t_offset),
                                 (uint32_t)bond, A.thr[bond]);
    if (pauli_has_x(code & 3)) atomicOr(&s_m[0], 1u << bond);
    if (pauli_has_x(code >> 2)) atomicOr(&s_m[1], 1u << bond);
    if (pauli_has_z(code & 3)) atomicOr(&s_m[2], 1u << bond);
    if (pauli_has_z(code >> 2)) atomicOr(&s_m[3], 1u << bond);
  }
  __syncthreads();
  // site i carries (right part of bond i-1) (left part of bond i)
  const uint32_t site_x = (s_m[1] << 1) ^ s_m[0];
  const uint32_t site_z = (s_m[3] << 1) ^ s_m[2];
  double* row = A.vals + ((int64_t)b * A.T + t) * (3 * L);
  for (int e = (int)threadIdx.x; e < 3 * L - 1; e += 64) {
    uint32_t flip;
    if (e < L)
      flip = (site_x >> e) & 1u;  // Z_e
    else if (e < 2 * L - 1)
      flip = ((site_x >> (e - L)) ^ (site_x >> (e - L + 1))) & 1u;  // Z_i Z_i+1, i = e - L
    else
      flip = (site_z >> (e - (2 * L - 1))) & 1u;  // X_i, i = e - (2 L - 1)
    if (flip) row[1 + e] = -row[1 + e];
  }
}

}  // namespace

hipError_t launch_bond_obs_sign(const BondObsArgs& a, hipStream_t stream) {
  if (a.batch < 1 || a.L < 2 || a.L > 32 || a.T < 1 || a.t_offset < 0 || a.n_traj < 1 ||
      !a.vals || !a.thr || (int64_t)a.batch * a.T > 0x7FFFFFFFll)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(bond_obs_sign_kernel, dim3((unsigned)((int64_t)a.batch * a.T)), dim3(64), 0,
                     stream, a);
  return hipGetLastError();
}

hipError_t launch_bond_diag(const BondDiagArgs& a, hipStream_t stream) {
  if (a.batch < 1 || a.L < 2 || a.L > 32 || a.n_traj < 1 || !a.out || !a.h || !a.phi || !a.thr ||
      a.diag_stride != (a.n_chunks + a.L_eff) * 64)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(bond_diag_kernel, dim3((unsigned)a.batch), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace dtc
