// dtc_rdm.h -- index algebra of the reduced density matrices (include/dtc.h
// dtc_rdm), shared by the kernels (dtc_rdm.hip) and the host reference
// (dtc_rdm_state, dtc_engine.cpp).  No device code, no HIP headers: a host
// compiler takes it as it is.
//
// A window is k sites s_0 < ... < s_{k-1}; row index alpha has bit m = the bit
// of site s_m, and rho[alpha][alpha'] = sum_c psi(alpha, c) conj psi(alpha', c)
// over the other bits c.  The kernels always work on four row bits: the window's
// sites (row bits 0 .. k-1) and, as row bits k .. 3, the lowest 4 - k bit
// positions of [0, L_eff) outside the window (the pad bits).  They form the
// 16 x 16 Gram matrix G over those bits, and rho is its block trace over the pad:
//   rho[alpha][alpha'] = sum_pi G[alpha | pi << k][alpha' | pi << k].
//
// The other L_eff - 4 bits, in ascending position, are the column index: its
// lowest 8 bits lie inside a tile of 4096 amplitudes, the rest number the tiles.
// Column bits 6, 7 number the workgroup's four waves; a wave's 1024 amplitudes
// span the four row bits and column bits 0 .. 5.  These ten positions always
// contain 0 .. 5 (a position below 6 is a row bit or one of the six lowest
// column bits), so the lanes take positions 0 .. 5 -- every load instruction
// reads 1 KiB of consecutive amplitudes -- and a thread's 16 registers take the
// other four (hi_pos).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define DTC_RDM_HD __host__ __device__
#else
#define DTC_RDM_HD
#endif

namespace dtc {
namespace rdm {

static constexpr int kRowBits = 4;        // window + pad
static constexpr int kRows = 16;
static constexpr int kTileBits = 12;      // = kTileBits (dtc_kernels.h)
static constexpr int kWaveBits = 10;      // row bits + column bits 0..5
static constexpr int kWaveColBits = 6;
static constexpr int kMaxK = 4;
static constexpr int kPartial = 512;      // per (state, workgroup): acc_re | acc_x
static constexpr int kMaxTilesPerWg = 8;

// Consecutive tiles one workgroup owns: a function of L_eff alone.
DTC_RDM_HD constexpr int64_t tiles_per_wg(int L_eff) {
  return L_eff - kTileBits >= 3 ? kMaxTilesPerWg : (int64_t)1 << (L_eff - kTileBits);
}
DTC_RDM_HD constexpr int64_t n_workgroups(int L_eff) {
  return ((int64_t)1 << (L_eff - kTileBits)) / tiles_per_wg(L_eff);
}

// nullptr, or what is wrong with the window
inline const char* check_window(const int32_t* sites, int k, int L) {
  if (!sites) return "null sites";
  if (k < 1 || k > kMaxK) return "window size k must be in [1, 4]";
  if (k > L) return "window size k exceeds L";
  for (int m = 0; m < k; ++m) {
    if (sites[m] < 0 || sites[m] >= L) return "window site outside [0, L)";
    if (m && sites[m] <= sites[m - 1]) return "window sites must be strictly ascending";
  }
  return nullptr;
}

// c with a zero bit inserted at each of the n ascending positions
DTC_RDM_HD inline uint64_t spread_cols(uint64_t c, const int* sorted, int n) {
  for (int i = 0; i < n; ++i) {
    const int r = sorted[i];
    c = ((c >> r) << (r + 1)) | (c & (((uint64_t)1 << r) - 1));
  }
  return c;
}

// bit m of a placed at pos[m]
DTC_RDM_HD inline uint64_t row_offset(int a, const int* pos, int n) {
  uint64_t x = 0;
  for (int m = 0; m < n; ++m) x |= (uint64_t)((a >> m) & 1) << pos[m];
  return x;
}

// A wave keeps amplitude (row a, wave column c6) at double u ^ swizzle(u) of its
// LDS slab, u = a | c6 << 4.  The MFMA operand read of k-step s (lane l: row
// l & 15, column 4 s + (l >> 4)) is u = l | s << 6: 64 consecutive doubles,
// permuted.  The XOR with column bits 1..4 spreads the writes of a high window
// (lanes = columns, 16 doubles apart) over the banks.  GF(2)-linear in u.
DTC_RDM_HD constexpr int lds_slot(int u) { return u ^ ((u >> 5) & 15); }

struct Geom {
  int k;
  int pos[kRowBits];      // row bit m -> bit position (window sites, then pad)
  int sorted[kRowBits];   // the same positions, ascending
  int hi_pos[4];          // positions 6 .. 9 (ascending) of a wave's ten: register bits
  int ushift[kWaveBits];  // bit of u = a | c6 << 4 held by the wave's n-th position
};

// sites checked by check_window against L <= L_eff, L_eff >= 12
inline Geom geometry(const int32_t* sites, int k, int L_eff) {
  Geom g{};
  g.k = k;
  uint64_t rows = 0;
  for (int m = 0; m < k; ++m) {
    g.pos[m] = sites[m];
    rows |= (uint64_t)1 << sites[m];
  }
  for (int p = 0, m = k; m < kRowBits; ++p)
    if (!((rows >> p) & 1)) {
      g.pos[m++] = p;
      rows |= (uint64_t)1 << p;
    }
  // ascending walk over the positions: row bits, and the six lowest column bits
  int n_sorted = 0, n_col = 0, n = 0;
  for (int p = 0; p < L_eff && n < kWaveBits; ++p) {
    int u;
    if ((rows >> p) & 1) {
      g.sorted[n_sorted++] = p;
      int m = 0;
      while (g.pos[m] != p) ++m;
      u = m;
    } else {
      if (n_col >= kWaveColBits) continue;
      u = kRowBits + n_col++;
    }
    g.ushift[n] = u;
    if (n >= 6) g.hi_pos[n - 6] = p;
    ++n;
  }
  return g;
}

}  // namespace rdm
}  // namespace dtc
