// dtc_corr.hip -- all-pair correlators (include/dtc.h dtc_correlations): Z_i
// and C_ij = <Z_i Z_j> of every state of a batch in HBM, from one streaming
// read of the batch.
//
// The sums are Walsh coefficients of |psi|^2 at masks of weight 0, 1 and 2
// (dtc_corr.h), formed in a hierarchy that is a fixed function of the logical
// index alone, so a row has the same bits in either batch layout, for any batch
// size:
//   * corr_chunk_kernel: the 79 coefficients of the 12 bits of chunk c (kTile
//     consecutive logical amplitudes).  Thread t holds amplitudes
//     c kTile + 256 j + t, j = 0..15 (sample_weights_kernel's index map): chunk
//     bits 8..11 are the register index, 0..5 the lane, 6..7 the wave.  A
//     16-point transform in registers gives the total s, the four singles r_k
//     and the six pairs r_kl of the register bits; the six-stage lane transform
//     of s and of each r_k leaves the coefficient of lane mask m in lane m;
//     the r_kl need their wave totals only.  Each wave writes its 56 kept
//     values to LDS, and after one barrier 79 threads combine the four waves
//     with the signs of bits 6, 7.  No atomics.
//   * corr_reduce_kernel: one workgroup per (state, output).  Thread t adds the
//     signed terms of chunks t, t + 256, ... in four interleaved accumulators,
//     wave_sum adds the 64 lanes, the four waves are added in order.
#include <hip/hip_runtime.h>

#include "dtc_corr.h"
#include "dtc_device.h"
#include "dtc_kernels.h"

namespace dtc {

namespace {

__device__ __forceinline__ double norm2(d2v a) { return a.x * a.x + a.y * a.y; }

// lane m ends with sum over lanes l of (-1)^popcount(l & m) h(l)
__device__ __forceinline__ double lane_wht(double h) {
  h = wht_stage<1>(h);
  h = wht_stage<2>(h);
  h = wht_stage<4>(h);
  h = wht_stage<8>(h);
  h = wht_stage<16>(h);
  h = wht_stage<32>(h);
  return h;
}

bool corr_args_ok(const CorrArgs& a) {
  return a.state && a.partial && a.z && (a.zz || a.L < 2) && a.batch >= 1 && a.batch <= 65535 &&
         a.L_eff >= kTileBits && a.L_eff <= 32 && a.L >= 1 && a.L <= a.L_eff &&
         a.octet_bits >= 0 && a.out_stride >= 0;
}

}  // namespace

__global__ __launch_bounds__(kThreads) void corr_chunk_kernel(CorrArgs A) {
  static_assert(kThreads == 256 && kWaveSize == 64 && kRegs == 16 && kTileBits == corr::kChunkBits,
                "chunk bits: lane 0..5, wave 6..7, register 8..11");
  __shared__ double s_v[kThreads / kWaveSize][corr::kWaveSlots];
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
  double p[kRegs];
#pragma unroll
  for (int j = 0; j < kRegs; ++j) p[j] = norm2(v[j]);
  // register bits: p[m] <- coefficient at register mask m
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int j = 0; j < kRegs; ++j) {
      if (j & (1 << q)) continue;
      const double u = p[j], w = p[j | (1 << q)];
      p[j] = u + w;
      p[j | (1 << q)] = u - w;
    }
  }
  const int lane = t & (kWaveSize - 1);
  double* sv = s_v[t / kWaveSize];
  {
    const double h = lane_wht(p[0]);
    const int slot = corr::slot_of_mask(lane);
    if (slot >= 0) sv[slot] = h;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double h = lane_wht(p[1 << k]);
    const int slot = corr::slot_of_mask(lane | (1 << (8 + k)));
    if (slot >= 0) sv[slot] = h;
  }
  {
    // the register pairs in the order of pair_index(4, k, l); lane 8 n ends
    // with the wave sum of vector n (wave_sum_multi)
    const double x[8] = {p[3], p[5], p[9], p[6], p[10], p[12], 0.0, 0.0};
    const double w = wave_sum_multi<8>(x);
    if ((lane & 7) == 0 && (lane >> 3) < 6) sv[50 + (lane >> 3)] = w;
  }
  __syncthreads();
  if (t < corr::kPartial) {
    const int m = corr::partial_mask(t);
    const int slot = corr::slot_of_mask(m & ~corr::kWaveBitMask);
    A.partial[((int64_t)b * n_chunks + c) * corr::kPartial + t] =
        corr::wave_combine((m >> 6) & 3, s_v[0][slot], s_v[1][slot], s_v[2][slot], s_v[3][slot]);
  }
}

__global__ __launch_bounds__(kThreads) void corr_reduce_kernel(CorrArgs A) {
  __shared__ double s_w[kThreads / kWaveSize];
  const int t = (int)threadIdx.x;
  const int o = (int)blockIdx.x;
  const int b = (int)blockIdx.y;
  const int64_t n_chunks = (int64_t)1 << (A.L_eff - kTileBits);
  const corr::Source src = corr::output_source(A.L, o);
  const double* part = A.partial + (int64_t)b * n_chunks * corr::kPartial;
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t c0 = t; c0 < n_chunks; c0 += 4 * kThreads) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t c = c0 + (int64_t)u * kThreads;
      if (c < n_chunks) a[u] += corr::term(part + c * corr::kPartial, src, (uint64_t)c);
    }
  }
  double acc = wave_sum((a[0] + a[1]) + (a[2] + a[3]));
  if ((t & (kWaveSize - 1)) == 0) s_w[t / kWaveSize] = acc;
  __syncthreads();
  if (t == 0) {
    acc = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
    if (o < A.L) A.z[(int64_t)b * A.out_stride + o] = acc;
    else A.zz[(int64_t)b * A.out_stride + (o - A.L)] = acc;
  }
}

hipError_t launch_corr_chunk(const CorrArgs& a, hipStream_t stream) {
  if (!corr_args_ok(a)) return hipErrorInvalidValue;
  const unsigned n_chunks = 1u << (a.L_eff - kTileBits);
  hipLaunchKernelGGL(corr_chunk_kernel, dim3(n_chunks, (unsigned)a.batch), dim3(kThreads), 0,
                     stream, a);
  return hipGetLastError();
}

hipError_t launch_corr_reduce(const CorrArgs& a, hipStream_t stream) {
  if (!corr_args_ok(a) || a.out_stride < a.L) return hipErrorInvalidValue;
  const unsigned n_out = (unsigned)(a.L + corr::n_pairs(a.L));
  hipLaunchKernelGGL(corr_reduce_kernel, dim3(n_out, (unsigned)a.batch), dim3(kThreads), 0, stream,
                     a);
  return hipGetLastError();
}

}  // namespace dtc
