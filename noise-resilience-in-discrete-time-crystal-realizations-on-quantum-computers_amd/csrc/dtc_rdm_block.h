// dtc_rdm_block.h -- index algebra of the reduced density matrices of blocks of
// contiguous sites (include/dtc.h dtc_rdm_block_sums), shared by the kernels
// (dtc_rdm_block.hip), the host reference (dtc_rdm_block_state, dtc_engine.cpp)
// and tools/rdm_block_geometry_check.cpp.  No device code, no HIP headers: a
// host compiler takes it as it is.
//
// A block is the k sites a .. a + k - 1, 5 <= k <= 10; row index alpha has bit m
// = the bit of site a + m, and rho[alpha][alpha'] = sum_c psi(alpha, c)
// conj psi(alpha', c) over the other bits c.  The kernels work on ke = max(k, 6)
// row bits at positions ae .. ae + ke - 1: a five-site block takes one adjacent
// pad bit, above the block where the state has one (ae = a, the pad is row bit
// 5), else below it (ae = a - 1, the pad is row bit 0), and rho is the block
// trace of the 64 x 64 Gram matrix over the pad.  With de = 2^ke the kernels
// form G[r][r'] = sum_c psi(r, c) conj psi(r', c), c the other L_eff - ke bits in
// ascending position:
//   amplitude(r, c) = (c >> ae) << (ae + ke) | r << ae | c & (2^ae - 1).
//
// Tiles.  G is cut into panels of 64 consecutive rows; a workgroup owns one
// lower-triangle tile (p, q), q <= p, of 64 x 64 entries, and one of n_split
// equal ranges of the column chunks.  A chunk is 64 consecutive columns.  One
// panel of one chunk is 4096 amplitudes with 12 local bits v: with m =
// min(ae, 6), the low m column bits (positions 0 .. m-1), the panel's six row
// bits (positions ae .. ae+5), then the other 6 - m column bits: ascending in
// position.  A thread's lane is v's bits 0..5, which are positions 0..5 of the
// chunk whatever ae is (the m column bits and, for ae < 6, the lowest row bits
// are contiguous from position 0; for ae >= 6 they are column bits 0..5).  So
// every staged load instruction reads 64 consecutive amplitudes, a 1 KiB run,
// for every start: the property the 64-row panels are there for.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define DTC_RDMB_HD __host__ __device__
#else
#define DTC_RDMB_HD
#endif

namespace dtc {
namespace rdmb {

static constexpr int kMinK = 5, kMaxK = 10;
static constexpr int kPanelBits = 6, kPanel = 64;   // rows of a panel
static constexpr int kChunkBits = 6, kChunk = 64;   // columns of a chunk
static constexpr int kLocalBits = 12;               // a panel of a chunk
static constexpr int kTargetWg = 64;                // workgroups per state wanted

// nullptr, or what is wrong with the block
inline const char* check_block(int start, int k, int L) {
  if (L < 1 || L > 32) return "L must be in [1, 32]";
  if (k < kMinK || k > kMaxK) return "block size k must be in [5, 10]";
  if (2 * k > L) return "block size k must be at most L / 2";
  if (start < 0) return "block start must be >= 0";
  if (start + k > L) return "block exceeds the chain: start + k > L";
  return nullptr;
}

struct Geom {
  int k, start;      // the block
  int ke, ae;        // the kernel's row bits: ke of them from position ae
  int pad_shift;     // k = 5: row index of alpha, pad pi is (alpha << pad_shift) | pi << pad_bit
  int pad_bit;       //        (pad above: shift 0, bit 5; pad below: shift 1, bit 0); else 0, 0
  int n_pad;         // 2 for k = 5, else 1
  int n_panels;      // 2^(ke - 6)
  int n_tiles;       // n_panels (n_panels + 1) / 2
  int n_chunks;      // 2^(L_eff - ke - 6)
  int n_split;       // column ranges per tile: a function of (L_eff, k) alone
  int m;             // min(ae, 6)
};

// block checked by check_block against L <= L_eff, L_eff >= 12
DTC_RDMB_HD inline Geom geometry(int start, int k, int L_eff) {
  Geom g{};
  g.k = k;
  g.start = start;
  g.ke = k < kPanelBits ? kPanelBits : k;
  g.ae = start;
  g.n_pad = 1 << (g.ke - k);
  if (g.ke > k) {
    if (start + g.ke <= L_eff) {
      g.pad_shift = 0;
      g.pad_bit = k;
    } else {
      g.ae = start - 1;
      g.pad_shift = 1;
      g.pad_bit = 0;
    }
  }
  g.n_panels = 1 << (g.ke - kPanelBits);
  g.n_tiles = g.n_panels * (g.n_panels + 1) / 2;
  g.n_chunks = 1 << (L_eff - g.ke - kChunkBits);
  g.m = g.ae < 6 ? g.ae : 6;
  // splits: enough workgroups per state, at least four chunks each where there
  // are that many, and the partials no larger than the state (2^(L_eff - 2 ke))
  int s = 1;
  while (g.n_tiles * s < kTargetWg) s <<= 1;
  const int by_chunks = g.n_chunks >= 4 ? g.n_chunks / 4 : 1;
  const int by_mem = 1 << (L_eff - 2 * g.ke);
  if (s > by_chunks) s = by_chunks;
  if (s > by_mem) s = by_mem;
  g.n_split = s < 1 ? 1 : s;
  return g;
}

// the kernel's row index of block row alpha and pad value pi
DTC_RDMB_HD inline int padded_row(const Geom& g, int alpha, int pi) {
  return (alpha << g.pad_shift) | (pi << g.pad_bit);
}

// amplitude index of (row r of ke bits, column c)
DTC_RDMB_HD inline uint64_t amp_index(int ae, int ke, uint64_t r, uint64_t c) {
  return ((c >> ae) << (ae + ke)) | (r << ae) | (c & (((uint64_t)1 << ae) - 1));
}

// a panel of a chunk: local index v (12 bits) -> row within the panel, column
// within the chunk
DTC_RDMB_HD inline int local_row(int v, int m) { return (v >> m) & (kPanel - 1); }
DTC_RDMB_HD inline int local_col(int v, int m) {
  return (v & ((1 << m) - 1)) | ((v >> (m + kPanelBits)) << m);
}

// LDS double of (row within the panel, column within the chunk): column-major
// with the row XORed by a function of the column.  The MFMA operand read of
// k-step s and 16-row block rb (lane l: row 16 rb + (l & 15), column 4 s +
// (l >> 4)) touches every bank pair twice, the minimum for 64 doubles; the
// staging write of a run of 64 columns of one row (ae >= 6) likewise.
// GF(2)-linear in (row, col).
DTC_RDMB_HD inline int lds_slot(int row, int col) {
  return (col << kPanelBits) | (row ^ col ^ ((col & 1) << 4));
}

// tile t of the lower triangle -> (p, q), q <= p, rows first: 0 -> (0,0),
// 1 -> (1,0), 2 -> (1,1), ...
DTC_RDMB_HD inline void tile_pq(int t, int& p, int& q) {
  p = 0;
  while (t > p) {
    t -= p + 1;
    ++p;
  }
  q = t;
}

}  // namespace rdmb
}  // namespace dtc
