// dtc_corr.h -- index algebra of the all-pair correlators (include/dtc.h
// dtc_correlations), shared by the kernels (dtc_corr.hip) and the host
// reference (dtc_correlations_state, dtc_engine.cpp).  No device code, no HIP
// headers: a host compiler takes it as it is.
//
// With z_i(x) = +1 / -1 for bit i of x clear / set, the observables of a state
// psi are Walsh coefficients of its probability vector at masks of weight 0, 1
// and 2:
//   W = sum_x |psi_x|^2,  Z_i = sum_x |psi_x|^2 z_i(x),
//   C_ij = sum_x |psi_x|^2 z_i(x) z_j(x).
// They are split at the chunk of 2^12 consecutive logical amplitudes:
//   * a chunk's partial holds the 79 coefficients of its own 12 bits: the total,
//     12 singles, 66 pairs (partial_mask);
//   * the bits 12 .. of a mask are signs of the chunk index c, applied when the
//     partials are combined (source, term).
// Inside a chunk, bits 6 and 7 number the workgroup's four waves; a wave keeps
// the 56 coefficients of the other ten bits (slot_of_mask) and the four waves
// are combined with the signs of bits 6, 7 (wave_combine).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define DTC_CORR_HD __host__ __device__
#else
#define DTC_CORR_HD
#endif

namespace dtc {
namespace corr {

static constexpr int kChunkBits = 12;      // = kTileBits (dtc_kernels.h)
static constexpr int kPartial = 79;        // per (state, chunk): 1 + 12 + 66
static constexpr int kOffSingle = 1;       // partial[1 + k]: bit k of the chunk
static constexpr int kOffPair = 13;        // partial[13 + pair_index(12, k, l)]
static constexpr int kWaveSlots = 56;      // per wave: 22 + 4 * 7 + 6
static constexpr int kWaveBitMask = 0xC0;  // chunk bits 6, 7: the wave index

DTC_CORR_HD constexpr int n_pairs(int n) { return n * (n - 1) / 2; }

// Pair (i, j), i < j < n, in row-major order (0,1), (0,2), ..., (n-2,n-1).
DTC_CORR_HD constexpr int pair_index(int n, int i, int j) {
  return i * (2 * n - i - 1) / 2 + (j - i - 1);
}

DTC_CORR_HD inline void pair_sites(int n, int idx, int& i, int& j) {
  i = 0;
  while (idx >= n - 1 - i) {
    idx -= n - 1 - i;
    ++i;
  }
  j = i + 1 + idx;
}

DTC_CORR_HD inline int popc(uint32_t m) { return __builtin_popcount(m); }
DTC_CORR_HD inline int lowbit(uint32_t m) { return __builtin_ctz(m); }

// Entry o of a chunk partial is the coefficient at this mask of the chunk's bits.
DTC_CORR_HD inline int partial_mask(int o) {
  if (o == 0) return 0;
  if (o < kOffPair) return 1 << (o - kOffSingle);
  int k, l;
  pair_sites(kChunkBits, o - kOffPair, k, l);
  return (1 << k) | (1 << l);
}

// Where a wave keeps the coefficient at mask m of the ten chunk bits that are
// not wave bits (lane bits 0..5, register bits 8..11), -1: not kept.
//   0: total; 1 + a: lane bit a; 7 + pair_index(6, a, b): lane pair;
//   22 + 7 k: register bit 8 + k; 23 + 7 k + a: lane a x register k;
//   50 + pair_index(4, k, l): register pair.
DTC_CORR_HD inline int slot_of_mask(int m) {
  if (m & kWaveBitMask) return -1;
  const uint32_t ml = (uint32_t)m & 63u, mr = ((uint32_t)m >> 8) & 15u;
  const int wl = popc(ml), wr = popc(mr);
  if (wl + wr > 2) return -1;
  if (wr == 0) {
    if (wl == 0) return 0;
    const int a = lowbit(ml);
    if (wl == 1) return 1 + a;
    return 7 + pair_index(6, a, lowbit(ml & (ml - 1)));
  }
  const int k = lowbit(mr);
  if (wr == 1) return 22 + 7 * k + (wl ? 1 + lowbit(ml) : 0);
  return 50 + pair_index(4, k, lowbit(mr & (mr - 1)));
}

// The coefficient at a chunk mask with wave bits `kind` = (mask >> 6) & 3 from
// the four waves' values of slot_of_mask(mask & ~kWaveBitMask): wave w holds
// chunk bits (7, 6) = w.  One fixed order.
DTC_CORR_HD inline double wave_combine(int kind, double v0, double v1, double v2, double v3) {
  const double a = (kind & 1) ? v0 - v1 : v0 + v1;
  const double b = (kind & 1) ? v2 - v3 : v2 + v3;
  return (kind & 2) ? a - b : a + b;
}

// An output -- site i (j < 0) or pair i < j -- as a column of the chunk
// partials and a sign mask over the chunk index c: the output is the sum over
// c of term(partial_c, source, c).
struct Source {
  int col;
  uint64_t gmask;
};

DTC_CORR_HD inline Source source(int i, int j) {
  Source s{0, 0};
  if (j < 0) {
    if (i < kChunkBits) s.col = kOffSingle + i;
    else s.gmask = (uint64_t)1 << (i - kChunkBits);
    return s;
  }
  if (j < kChunkBits) {
    s.col = kOffPair + pair_index(kChunkBits, i, j);
    return s;
  }
  s.gmask = (uint64_t)1 << (j - kChunkBits);
  if (i < kChunkBits) s.col = kOffSingle + i;
  else s.gmask |= (uint64_t)1 << (i - kChunkBits);
  return s;
}

DTC_CORR_HD inline double term(const double* partial_c, Source s, uint64_t c) {
  const double v = partial_c[s.col];
  return __builtin_parityll(c & s.gmask) ? -v : v;
}

// Output o of a state of n sites: o < n is site o, then the pairs in order.
DTC_CORR_HD inline Source output_source(int n, int o) {
  if (o < n) return source(o, -1);
  int i, j;
  pair_sites(n, o - n, i, j);
  return source(i, j);
}

}  // namespace corr
}  // namespace dtc
