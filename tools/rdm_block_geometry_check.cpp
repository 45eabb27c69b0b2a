// rdm_block_geometry_check.cpp -- host check of the block density-matrix
// kernels' index algebra (csrc/dtc_rdm_block.h), compiled and run by
// tests/test_rdm_block_cpu.py.
//
// For every block (start, k), 5 <= k <= 10, 2 k <= L_eff, of L_eff = 12 .. 20 it
// walks the Gram kernel's own addressing -- panel, chunk, thread, register -- and
// checks that every amplitude of the state is read exactly once per sweep of the
// panels and in bounds, that the address is the sum of the panel's, the chunk's,
// the thread's and the register's parts as the kernel forms it, that the row the
// kernel assigns is the block's (with the pad bit of a five-site block), that
// every load instruction of a wave reads 64 consecutive amplitudes, that the LDS
// slots of a panel of a chunk are distinct and linear over the local index, that
// an MFMA operand read touches every pair of banks exactly twice, that the
// tiles enumerate the lower triangle once, and that the splits divide the
// chunks with partials no larger than the state.  Prints "cases N fails M";
// exit status 1 on any failure.
#include <cstdint>
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "dtc_rdm_block.h"

using namespace dtc::rdmb;

int main() {
  long fails = 0, cases = 0;
  const int kThreads = 512, kRegs = (1 << kLocalBits) / kThreads;
  for (int L_eff = 12; L_eff <= 20; ++L_eff)
    for (int k = kMinK; k <= kMaxK && 2 * k <= L_eff; ++k)
      for (int start = 0; start + k <= L_eff; ++start) {
        if (check_block(start, k, L_eff)) {
          ++fails;
          continue;
        }
        const Geom g = geometry(start, k, L_eff);
        ++cases;
        const int de = 1 << g.ke, d = 1 << k;
        fails += g.ae < 0 || g.ae + g.ke > L_eff || g.n_pad * d != de;
        fails += g.n_panels * kPanel != de;
        fails += g.n_chunks * kChunk != (1 << (L_eff - g.ke));
        fails += g.n_split < 1 || g.n_chunks % g.n_split != 0;
        fails += ((uint64_t)g.n_split << (2 * g.ke)) > ((uint64_t)1 << L_eff);
        // tiles: the lower triangle once
        std::set<std::pair<int, int>> tiles;
        for (int t = 0; t < g.n_tiles; ++t) {
          int p, q;
          tile_pq(t, p, q);
          fails += q > p || p >= g.n_panels || q < 0;
          tiles.insert({p, q});
        }
        fails += (int)tiles.size() != g.n_tiles;
        std::vector<char> seen((size_t)1 << L_eff, 0);
        for (int p = 0; p < g.n_panels; ++p)
          for (int ch = 0; ch < g.n_chunks; ++ch) {
            const uint64_t base = amp_index(g.ae, g.ke, (uint64_t)p << kPanelBits, 0) +
                                  amp_index(g.ae, g.ke, 0, (uint64_t)ch << kChunkBits);
            // (the LDS walk is the same for every panel and chunk: once)
            const bool lds = p == 0 && ch == 0;
            std::set<int> slots;
            for (int j = 0; j < kRegs; ++j)
              for (int t = 0; t < kThreads; ++t) {
                const int v = t | (j << 9);
                const int lr = local_row(v, g.m), lc = local_col(v, g.m);
                const uint64_t r = ((uint64_t)p << kPanelBits) | (uint64_t)lr;
                const uint64_t c = ((uint64_t)ch << kChunkBits) | (uint64_t)lc;
                const uint64_t x = amp_index(g.ae, g.ke, r, c);
                if (x >> L_eff) {
                  ++fails;
                  continue;
                }
                fails += seen[x];
                seen[x] = 1;
                const uint64_t parts =
                    base + amp_index(g.ae, g.ke, local_row(t, g.m), local_col(t, g.m)) +
                    amp_index(g.ae, g.ke, local_row(j << 9, g.m), local_col(j << 9, g.m));
                fails += parts != x;
                // a wave's load: lane l reads the wave's first amplitude + l
                if ((t & 63) != 0) {
                  const int v0 = (t & ~63) | (j << 9);
                  const uint64_t x0 =
                      amp_index(g.ae, g.ke, ((uint64_t)p << kPanelBits) | local_row(v0, g.m),
                                ((uint64_t)ch << kChunkBits) | local_col(v0, g.m));
                  fails += x != x0 + (uint64_t)(t & 63) || (x0 & 63) != 0;
                }
                // the row is the block's: alpha and the pad bit
                const int alpha = g.n_pad == 1 ? (int)r
                                               : (g.pad_shift ? (int)(r >> 1) : (int)(r & (d - 1)));
                const int pi = g.n_pad == 1 ? 0 : (int)((r >> g.pad_bit) & 1);
                fails += padded_row(g, alpha, pi) != (int)r;
                fails += (int)((x >> start) & (uint64_t)(d - 1)) != alpha;
                if (lds) {
                  const int slot = lds_slot(lr, lc);
                  fails += slot != (lds_slot(local_row(t, g.m), local_col(t, g.m)) ^
                                    lds_slot(local_row(j << 9, g.m), local_col(j << 9, g.m)));
                  fails += slot < 0 || slot >= kPanel * kChunk;
                  slots.insert(slot);
                }
              }
            if (lds) fails += slots.size() != (size_t)(kPanel * kChunk);
          }
        for (char c : seen) fails += !c;
      }
  // MFMA operand reads: lane l takes row 16 blk + (l & 15), column 4 s + (l >> 4)
  for (int blk = 0; blk < 4; ++blk)
    for (int s = 0; s < kChunk / 4; ++s) {
      int banks[32] = {0};
      for (int l = 0; l < 64; ++l) {
        const int row = 16 * blk + (l & 15), col = 4 * s + (l >> 4);
        const int slot = lds_slot(row, col);
        fails += slot != (lds_slot(row, l >> 4) ^ lds_slot(0, 4 * s));
        fails += lds_slot(row ^ 16, col) != (slot ^ 16);
        ++banks[slot & 31];
      }
      for (int b = 0; b < 32; ++b) fails += banks[b] != 2;
    }
  std::printf("cases %ld fails %ld\n", cases, fails);
  return fails != 0;
}
