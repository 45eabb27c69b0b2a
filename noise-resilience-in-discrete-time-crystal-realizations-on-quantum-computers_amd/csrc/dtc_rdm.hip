// dtc_rdm.hip -- reduced density matrices of site windows (include/dtc.h
// dtc_rdm): rho_A = M M^dagger of every state of a batch in HBM, M the state
// reshaped to the window's rows, from one streaming read of the batch per window.
//
// The kernels work on four row bits (the window's sites and pad bits, dtc_rdm.h)
// and form the 16 x 16 Gram matrix G[a][a'] = sum_c psi(a, c) conj psi(a', c):
//   * rdm_gram_kernel: a workgroup owns tiles_per_wg(L_eff) consecutive tiles of
//     4096 amplitudes (4 row bits x 8 column bits); wave w takes columns
//     64 w .. 64 w + 63 of each.  Lanes hold bit positions 0..5, so each of a
//     thread's 16 nontemporal loads is part of a 1 KiB run.  The wave moves the
//     real parts, then the imaginary parts, through its own 8 KiB LDS slab into
//     the MFMA operand layout (lane l: row l & 15, column 4 s + (l >> 4) of
//     k-step s; no workgroup barrier), and per k-step issues three
//     v_mfma_f64_16x16x4_f64 with A and B from the same registers:
//       acc_rr += R R^T,  acc_ii += I I^T,  acc_x += I R^T,
//     so that Re G = acc_rr + acc_ii and Im G = X - X^T.  The instruction sums
//     over the four columns of a k-step; nothing crosses lanes outside it.  The
//     four waves are added in order into one 512-double partial per workgroup.
//   * rdm_reduce_kernel: one workgroup per state adds the partials (entry t in
//     four interleaved accumulators over the workgroup index), takes the block
//     trace over the pad bits, forms X - X^T and writes the lower triangle and
//     its conjugate: Hermitian bit for bit, the diagonal's imaginary part 0.
// Every sum is a fixed function of the logical index: no atomics, the same bits
// in either batch layout and for any batch size.
#include <hip/hip_runtime.h>

#include "dtc_device.h"
#include "dtc_kernels.h"
#include "dtc_rdm.h"

namespace dtc {

namespace {

typedef double d4v __attribute__((ext_vector_type(4)));

// orders a wave's own LDS accesses: the slab is private to the wave
__device__ __forceinline__ void wave_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

bool rdm_args_ok(const RdmArgs& a) {
  if (!(a.state && a.partial && a.out && a.batch >= 1 && a.batch <= 65535 &&
        a.L_eff >= kTileBits && a.L_eff <= 32 && a.octet_bits >= 0 && a.g.k >= 1 &&
        a.g.k <= rdm::kMaxK && a.out_stride >= ((int64_t)2 << (2 * a.g.k))))
    return false;
  for (int m = 0; m < rdm::kRowBits; ++m)
    if (a.g.pos[m] < 0 || a.g.pos[m] >= a.L_eff || a.g.sorted[m] < 0 ||
        a.g.sorted[m] >= a.L_eff || (m && a.g.sorted[m] <= a.g.sorted[m - 1]))
      return false;
  for (int i = 0; i < 4; ++i)
    if (a.g.hi_pos[i] < 6 || a.g.hi_pos[i] >= a.L_eff) return false;
  for (int n = 0; n < rdm::kWaveBits; ++n)
    if (a.g.ushift[n] < 0 || a.g.ushift[n] >= rdm::kWaveBits) return false;
  return true;
}

}  // namespace

__global__ __launch_bounds__(kThreads) void rdm_gram_kernel(RdmArgs A) {
  static_assert(kThreads == 256 && kWaveSize == 64 && kRegs == 16 && kTileBits == rdm::kTileBits,
                "tile: 4 row bits x 8 column bits; a wave: 4 row bits x 6 column bits");
  __shared__ double s_t[kThreads / kWaveSize][1 << rdm::kWaveBits];
  const int t = (int)threadIdx.x;
  // (the wave index is uniform: a tile's base and the register offsets are scalar)
  const int lane = t & (kWaveSize - 1), w = __builtin_amdgcn_readfirstlane(t / kWaveSize);
  const int b = (int)blockIdx.y;
  const int64_t len = (int64_t)1 << A.L_eff;
  const double2* st = A.state + state_base(b, len, A.octet_bits);
  const int tpw = (int)rdm::tiles_per_wg(A.L_eff);

  // the lane's six positions and the registers' four, as LDS slots and offsets
  int u_lane = 0;
#pragma unroll
  for (int n = 0; n < 6; ++n) u_lane |= ((lane >> n) & 1) << A.g.ushift[n];
  const int slot_lane = rdm::lds_slot(u_lane);
  int slot_j[kRegs];
  int64_t off_j[kRegs];
  slot_j[0] = 0;
  off_j[0] = 0;
#pragma unroll
  for (int j = 1; j < kRegs; ++j) {
    const int i = __builtin_ctz(j), prev = j & (j - 1);
    slot_j[j] = slot_j[prev] ^ rdm::lds_slot(1 << A.g.ushift[6 + i]);
    off_j[j] = off_j[prev] + octet_spread((int64_t)1 << A.g.hi_pos[i], A.octet_bits);
  }
  const uint32_t lane_off = (uint32_t)octet_spread(lane, A.octet_bits) * (uint32_t)sizeof(double2);
  double* const sl = s_t[w];

  d4v acc_rr = {0.0, 0.0, 0.0, 0.0}, acc_ii = acc_rr, acc_x = acc_rr;
  for (int ti = 0; ti < tpw; ++ti) {
    const uint64_t tile = (uint64_t)blockIdx.x * tpw + ti;
    const int64_t x0 =
        (int64_t)rdm::spread_cols((tile << 8) | ((uint64_t)w << 6), A.g.sorted, rdm::kRowBits);
    const double2* src = st + octet_spread(x0, A.octet_bits);
    d2v v[kRegs];
#pragma unroll
    for (int j = 0; j < kRegs; ++j)
      v[j] = __builtin_nontemporal_load(
          (const d2v*)((const char*)(src + off_j[j]) + lane_off));
    double R[kRegs], I[kRegs];
    wave_order();
#pragma unroll
    for (int j = 0; j < kRegs; ++j) sl[slot_lane ^ slot_j[j]] = v[j].x;
    wave_order();
#pragma unroll
    for (int s = 0; s < kRegs; ++s) R[s] = sl[rdm::lds_slot(lane | (s << 6))];
    wave_order();
#pragma unroll
    for (int j = 0; j < kRegs; ++j) sl[slot_lane ^ slot_j[j]] = v[j].y;
    wave_order();
#pragma unroll
    for (int s = 0; s < kRegs; ++s) I[s] = sl[rdm::lds_slot(lane | (s << 6))];
#pragma unroll
    for (int s = 0; s < kRegs; ++s) {
      acc_rr = __builtin_amdgcn_mfma_f64_16x16x4f64(R[s], R[s], acc_rr, 0, 0, 0);
      acc_ii = __builtin_amdgcn_mfma_f64_16x16x4f64(I[s], I[s], acc_ii, 0, 0, 0);
      acc_x = __builtin_amdgcn_mfma_f64_16x16x4f64(I[s], R[s], acc_x, 0, 0, 0);
    }
  }

  // C/D of the f64 MFMA: register r of lane l is (row (l >> 4) + 4 r, col l & 15)
  wave_order();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int e = ((lane >> 4) + 4 * r) * rdm::kRows + (lane & 15);
    sl[e] = acc_rr[r] + acc_ii[r];
    sl[256 + e] = acc_x[r];
  }
  __syncthreads();
  double* part = A.partial + ((int64_t)b * gridDim.x + blockIdx.x) * rdm::kPartial;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int e = 256 * h + t;
    part[e] = ((s_t[0][e] + s_t[1][e]) + s_t[2][e]) + s_t[3][e];
  }
}

__global__ __launch_bounds__(kThreads) void rdm_reduce_kernel(RdmArgs A) {
  __shared__ double s_re[256], s_x[256];
  const int t = (int)threadIdx.x;
  const int b = (int)blockIdx.x;
  const int64_t n_wg = rdm::n_workgroups(A.L_eff);
  const double* part = A.partial + (int64_t)b * n_wg * rdm::kPartial;
  double re[4] = {0.0, 0.0, 0.0, 0.0}, xs[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t g0 = 0; g0 < n_wg; g0 += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (g0 + u >= n_wg) continue;
      re[u] += part[(g0 + u) * rdm::kPartial + t];
      xs[u] += part[(g0 + u) * rdm::kPartial + 256 + t];
    }
  }
  s_re[t] = (re[0] + re[1]) + (re[2] + re[3]);
  s_x[t] = (xs[0] + xs[1]) + (xs[2] + xs[3]);
  __syncthreads();
  const int k = A.g.k, d = 1 << k;
  const int al = t >> k, ap = t & (d - 1);
  if (al >= d || ap > al) return;
  double gr = 0.0, gi = 0.0;
  for (int pi = 0; pi < (rdm::kRows >> k); ++pi) {
    const int a = al | (pi << k), a2 = ap | (pi << k);
    gr += s_re[a * rdm::kRows + a2];
    gi += s_x[a * rdm::kRows + a2] - s_x[a2 * rdm::kRows + a];
  }
  double* out = A.out + (int64_t)b * A.out_stride;
  if (al == ap) {
    out[2 * (al * d + al)] = gr;
    out[2 * (al * d + al) + 1] = 0.0;
    return;
  }
  out[2 * (al * d + ap)] = gr;
  out[2 * (al * d + ap) + 1] = gi;
  out[2 * (ap * d + al)] = gr;
  out[2 * (ap * d + al) + 1] = -gi;
}

hipError_t launch_rdm_gram(const RdmArgs& a, hipStream_t stream) {
  if (!rdm_args_ok(a)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rdm_gram_kernel, dim3((unsigned)rdm::n_workgroups(a.L_eff), (unsigned)a.batch),
                     dim3(kThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_rdm_reduce(const RdmArgs& a, hipStream_t stream) {
  if (!rdm_args_ok(a)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rdm_reduce_kernel, dim3((unsigned)a.batch), dim3(kThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace dtc
