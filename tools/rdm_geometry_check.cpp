// rdm_geometry_check.cpp -- host check of the density-matrix kernels' index
// algebra (csrc/dtc_rdm.h), compiled and run by tests/test_rdm_cpu.py.
//
// For every window of 1..4 sites at L_eff = 12, 13 (a sample at 14, 15) it walks
// the Gram kernel's own addressing -- tile, wave, lane, register -- and checks
// that every amplitude of the state is read exactly once and in bounds, that the
// (row, column) the LDS slot stands for is the amplitude's, that a wave's 1024
// slots are distinct, and that the MFMA operand read of a k-step takes 64
// consecutive doubles.  Prints "cases N fails M"; exit status 1 on any failure.
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "dtc_rdm.h"

using namespace dtc::rdm;

int main() {
  long fails = 0, cases = 0;
  for (int L_eff = kTileBits; L_eff <= 15; ++L_eff)
    for (int k = 1; k <= kMaxK; ++k)
      for (uint64_t code = 0; code < ((uint64_t)1 << L_eff); ++code) {
        if (__builtin_popcountll(code) != k) continue;
        if (L_eff > 13 && (code % 7)) continue;
        int32_t sites[kMaxK];
        for (int p = 0, m = 0; p < L_eff; ++p)
          if ((code >> p) & 1) sites[m++] = p;
        if (check_window(sites, k, L_eff)) {
          ++fails;
          continue;
        }
        const Geom g = geometry(sites, k, L_eff);
        ++cases;
        for (int i = 0; i < k; ++i) fails += g.pos[i] != sites[i];
        for (int i = 1; i < kRowBits; ++i) fails += g.sorted[i] <= g.sorted[i - 1];
        for (int i = 0; i < 4; ++i) fails += g.hi_pos[i] < 6 || g.hi_pos[i] >= L_eff;
        // pad bits: the lowest positions outside the window
        for (int m = k, p = 0; m < kRowBits; ++p) {
          bool in_window = false;
          for (int i = 0; i < k; ++i) in_window = in_window || sites[i] == p;
          if (!in_window) fails += g.pos[m++] != p;
        }
        const int64_t n_tiles = (int64_t)1 << (L_eff - kTileBits);
        fails += n_workgroups(L_eff) * tiles_per_wg(L_eff) != n_tiles;
        std::vector<char> seen((size_t)1 << L_eff, 0);
        for (int64_t tile = 0; tile < n_tiles; ++tile)
          for (int w = 0; w < 4; ++w) {
            const uint64_t cw = ((uint64_t)tile << 8) | ((uint64_t)w << 6);
            const uint64_t x0 = spread_cols(cw, g.sorted, kRowBits);
            std::set<int> slots;
            for (int lane = 0; lane < 64; ++lane) {
              int u_lane = 0;
              for (int n = 0; n < 6; ++n) u_lane |= ((lane >> n) & 1) << g.ushift[n];
              for (int j = 0; j < 16; ++j) {
                int u_j = 0;
                uint64_t off = 0;
                for (int i = 0; i < 4; ++i)
                  if ((j >> i) & 1) {
                    u_j |= 1 << g.ushift[6 + i];
                    off += (uint64_t)1 << g.hi_pos[i];
                  }
                fails += (u_lane & u_j) != 0;
                const int u = u_lane | u_j;
                const uint64_t x = x0 + lane + off;
                if (x >> L_eff) {
                  ++fails;
                  continue;
                }
                fails += seen[x];
                seen[x] = 1;
                const uint64_t want =
                    spread_cols(cw | (uint64_t)(u >> 4), g.sorted, kRowBits) |
                    row_offset(u & 15, g.pos, kRowBits);
                fails += want != x;
                const int slot = lds_slot(u_lane) ^ lds_slot(u_j);
                fails += slot != lds_slot(u) || slot < 0 || slot >= (1 << kWaveBits);
                slots.insert(slot);
              }
            }
            fails += slots.size() != ((size_t)1 << kWaveBits);
          }
        for (char c : seen) fails += !c;
      }
  for (int s = 0; s < 16; ++s) {
    std::set<int> r;
    for (int l = 0; l < 64; ++l) {
      const int q = lds_slot(l | (s << 6));
      fails += q < 64 * s || q >= 64 * s + 64;
      r.insert(q);
    }
    fails += r.size() != 64;
  }
  std::printf("cases %ld fails %ld\n", cases, fails);
  return fails != 0;
}
