// dtc_sample.hip -- measurement sampling (include/dtc.h dtc_sample): bitstrings
// drawn from a batch of states in HBM.
//
// A sample of state psi for the uniform u is the smallest index x with
// S(x) > u W, S the running sum of |psi_y|^2 and W its total.  The sums are
// formed in a hierarchy that is a fixed function of the logical index alone,
// so a sample has the same bits in either batch layout, for any batch size:
//   * sample_weights_kernel: w[c] = sum over chunk c (kTile consecutive
//     logical amplitudes).  Thread t adds amplitudes c kTile + 256 j + t,
//     j = 0..15 in order (a wave's 64 lanes read one contiguous KiB, a run of
//     the octet layout), wave_sum adds the 64 lanes, the four waves are added
//     in order.  One streaming read of the batch, no atomics.
//   * sample_pick_kernel: one workgroup per (state, shot) narrows a range of
//     items (first the chunk weights, then the 4096 |a|^2 of the chosen chunk)
//     to one: the range is cut into 256 consecutive parts, thread t adds part t
//     in index order, thread 0 adds the 256 part sums in order and selects the
//     first part whose running sum exceeds the remainder; the remainder minus
//     the sum of the parts before it goes down to the next level.  W is the sum
//     of the first level's parts.  Sums of non-negative terms added in one
//     fixed order never decrease, so a part of zero weight is never selected;
//     where rounding leaves no part (u W rounds up to W, or a level's re-added
//     sum falls short of the weight selected above it) the last part of
//     non-zero weight is taken, down to the last non-zero amplitude.
#include <hip/hip_runtime.h>

#include "dtc_device.h"
#include "dtc_kernels.h"
#include "dtc_rng.h"

namespace dtc {

namespace {

__device__ __forceinline__ double norm2(d2v a) { return a.x * a.x + a.y * a.y; }

__global__ __launch_bounds__(kThreads) void sample_weights_kernel(SampleArgs A) {
  __shared__ double s_w[kThreads / kWaveSize];
  const int t = (int)threadIdx.x;
  const int64_t n_chunks = (int64_t)1 << (A.L_eff - kTileBits);
  const int64_t c = blockIdx.x;
  const int b = (int)blockIdx.y;
  const int64_t len = (int64_t)1 << A.L_eff;
  const double2* st = A.state + state_base(b, len, A.octet_bits);
  const int64_t x0 = c * kTile + t;
  d2v v[kRegs];
#pragma unroll
  for (int j = 0; j < kRegs; ++j)
    v[j] = __builtin_nontemporal_load(
        (const d2v*)(st + octet_spread(x0 + (int64_t)j * kThreads, A.octet_bits)));
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < kRegs; ++j) acc += norm2(v[j]);
  acc = wave_sum(acc);
  if ((t & (kWaveSize - 1)) == 0) s_w[t / kWaveSize] = acc;
  __syncthreads();
  if (t == 0) A.weights[(int64_t)b * n_chunks + c] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

// One level of the pick: items [lo, lo + n) -> the selected part of them.
// first: rem is the uniform u on entry and becomes u W - (sum before the part).
template <class Get>
__device__ __forceinline__ void narrow(Get get, int64_t& lo, int64_t& n, double& rem, bool first,
                                       double* s_sum, double* s_rem, int* s_sel) {
  const int t = (int)threadIdx.x;
  const int64_t per = (n + kThreads - 1) / kThreads;
  const int64_t i0 = (int64_t)t * per, i1 = i0 + per < n ? i0 + per : n;
  double acc = 0.0;
  for (int64_t i = i0; i < i1; ++i) acc += get(lo + i);
  s_sum[t] = acc;
  __syncthreads();
  if (t == 0) {
    double target = rem;
    if (first) {
      double w = 0.0;
      for (int i = 0; i < kThreads; ++i) w += s_sum[i];
      target = rem * w;
    }
    double run = 0.0;
    int sel = -1;
    for (int i = 0; i < kThreads; ++i) {
      const double nx = run + s_sum[i];
      if (nx > target) {
        sel = i;
        break;
      }
      run = nx;
    }
    if (sel < 0) {
      // rounding left no part: the last one of non-zero weight, and so on down
      sel = 0;
      for (int i = 0; i < kThreads; ++i)
        if (s_sum[i] > 0.0) sel = i;
      *s_rem = __builtin_huge_val();
    } else {
      *s_rem = target - run;
    }
    *s_sel = sel;
  }
  __syncthreads();
  const int sel = *s_sel;
  rem = *s_rem;
  lo += sel * per;
  n = (sel + 1) * per <= n ? per : n - sel * per;
  __syncthreads();  // s_sum, s_sel, s_rem are rewritten by the next level
}

__global__ __launch_bounds__(kThreads) void sample_pick_kernel(SampleArgs A) {
  __shared__ double s_sum[kThreads];
  __shared__ double s_rem;
  __shared__ int s_sel;
  const int shot = (int)blockIdx.x;
  const int b = (int)blockIdx.y;
  const int64_t gstate = A.batch_start + b;
  const uint64_t traj = (uint64_t)(A.traj_offset + gstate % A.n_traj);
  const int64_t n_chunks = (int64_t)1 << (A.L_eff - kTileBits);
  const int64_t len = (int64_t)1 << A.L_eff;
  const int og = A.octet_bits;
  double rem = sample_uniform(A.seed, traj, A.period, A.basis, (uint32_t)shot);
  bool first = true;
  // the chunk
  const double* w = A.weights + (int64_t)b * n_chunks;
  int64_t lo = 0, n = n_chunks;
  while (n > 1) {
    narrow([&](int64_t i) { return w[i]; }, lo, n, rem, first, s_sum, &s_rem, &s_sel);
    first = false;
  }
  // the amplitude within it
  const double2* st = A.state + state_base(b, len, og);
  lo *= kTile;
  n = kTile;
  while (n > 1) {
    narrow(
        [&](int64_t i) {
          const double2 a = st[octet_spread(i, og)];
          return a.x * a.x + a.y * a.y;
        },
        lo, n, rem, first, s_sum, &s_rem, &s_sel);
    first = false;
  }
  if (threadIdx.x == 0) A.out[(int64_t)b * A.out_stride + shot] = (uint64_t)lo;
}

bool sample_args_ok(const SampleArgs& a) {
  return a.state && a.weights && a.batch >= 1 && a.batch <= 65535 && a.L_eff >= kTileBits &&
         a.L_eff <= 32 && a.n_traj >= 1 && a.octet_bits >= 0;
}

}  // namespace

hipError_t launch_sample_weights(const SampleArgs& a, hipStream_t stream) {
  if (!sample_args_ok(a)) return hipErrorInvalidValue;
  const unsigned n_chunks = 1u << (a.L_eff - kTileBits);
  hipLaunchKernelGGL(sample_weights_kernel, dim3(n_chunks, (unsigned)a.batch), dim3(kThreads), 0,
                     stream, a);
  return hipGetLastError();
}

hipError_t launch_sample_pick(const SampleArgs& a, hipStream_t stream) {
  if (!sample_args_ok(a) || !a.out || a.n_shots < 1 || a.n_shots > (1 << 30) ||
      a.out_stride < a.n_shots || a.basis > 1u)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(sample_pick_kernel, dim3((unsigned)a.n_shots, (unsigned)a.batch),
                     dim3(kThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace dtc
