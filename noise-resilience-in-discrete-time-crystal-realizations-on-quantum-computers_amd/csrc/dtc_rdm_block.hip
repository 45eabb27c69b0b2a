// dtc_rdm_block.hip -- reduced density matrices of blocks of 5 .. 10 contiguous
// sites (include/dtc.h dtc_rdm_block_sums): the Hermitian rank update
// G = sum_c v_c v_c^dagger of every state of a batch, v_c the column c of the
// state reshaped to the block's rows (index algebra: dtc_rdm_block.h).
//
//   * rdm_block_gram_kernel: a workgroup of 512 threads owns one 64 x 64
//     lower-triangle tile (p, q) of G for one state and one of n_split ranges of
//     the column chunks.  Per chunk of 64 columns each thread loads 8 amplitudes
//     of row panel p and 8 of panel q (the diagonal tile: one panel) -- each load
//     instruction a 1 KiB run for every start -- and the workgroup runs four LDS
//     phases on two 32 KiB panels held column-major with an XOR swizzle
//     (rdmb::lds_slot):
//       [R_p | R_q] re += R_p R_q^T      [I_p | R_q] im += I_p R_q^T
//       [I_p | I_q] re += I_p I_q^T      [-R_p | I_q] im += (-R_p) I_q^T
//     each phase replacing one panel from the registers.  Wave w owns rows
//     16 (w >> 1) .. and columns 32 (w & 1) ..: per k-step of four columns one A
//     and two B operand reads feed two v_mfma_f64_16x16x4_f64 (lane l supplies
//     row l & 15, column l >> 4; C/D: col = l & 15, row = (l >> 4) + 4 reg).  The
//     diagonal tile's two waves above the diagonal are skipped.  The sums run
//     over the columns in an order fixed by (L_eff, k): no atomics.  The tile
//     goes, lower triangle only on the diagonal tile, into the state's partial
//     [split][de][de][2], or -- one split, no pad -- straight into the work
//     matrix with its conjugate mirrored.
//   * rdm_block_finish_kernel (splits or a pad bit): per entry of the lower
//     triangle the splits added in ascending order, the block trace over the pad
//     bit, and the entry and its conjugate into the work matrix [d][d][2].
//   * rdm_block_purity_kernel: sum |G|^2 of a work matrix, one workgroup per
//     state, thread t taking entries t + 256 i in four interleaved accumulators
//     and a fixed LDS tree: a function of the logical index alone.
// Work matrices are Hermitian bit for bit with an exactly real diagonal.
#include <hip/hip_runtime.h>

#include "dtc_device.h"
#include "dtc_kernels.h"
#include "dtc_rdm_block.h"

namespace dtc {

namespace {

typedef double d4v __attribute__((ext_vector_type(4)));

// the Gram kernel's workgroup: eight waves, two workgroups per CU
constexpr int kGramThreads = 512;
// amplitudes per thread and panel
constexpr int kGramRegs = (1 << rdmb::kLocalBits) / kGramThreads;

bool rdm_block_args_ok(const RdmBlockArgs& a) {
  const rdmb::Geom& g = a.g;
  if (!(a.batch >= 1 && a.batch <= 65535 && a.L_eff >= kTileBits && a.L_eff <= 32 &&
        a.octet_bits >= 0 && g.k >= rdmb::kMinK && g.k <= rdmb::kMaxK))
    return false;
  // the geometry is the header's own for this block: every index stays inside
  // the state, the partials and the work matrix
  if (g.start < 0 || g.start + g.k > a.L_eff || 2 * g.k > a.L_eff) return false;
  const rdmb::Geom want = rdmb::geometry(g.start, g.k, a.L_eff);
  return want.ke == g.ke && want.ae == g.ae && want.pad_shift == g.pad_shift &&
         want.pad_bit == g.pad_bit && want.n_pad == g.n_pad && want.n_panels == g.n_panels &&
         want.n_tiles == g.n_tiles && want.n_chunks == g.n_chunks && want.n_split == g.n_split &&
         want.m == g.m && g.ae >= 0 && g.ae + g.ke <= a.L_eff;
}

}  // namespace

__global__ __launch_bounds__(kGramThreads, 4) void rdm_block_gram_kernel(RdmBlockArgs A) {
  static_assert(kGramThreads == 512 && kWaveSize == 64,
                "eight waves: 16 x 32 each of a 64 x 64 tile");
  __shared__ double s_a[rdmb::kPanel * rdmb::kChunk], s_b[rdmb::kPanel * rdmb::kChunk];
  const int t = (int)threadIdx.x;
  const int lane = t & (kWaveSize - 1), w = __builtin_amdgcn_readfirstlane(t / kWaveSize);
  const int wr = w >> 1, wc = w & 1;  // rows 16 wr .., columns 32 wc ..
  const int b = (int)blockIdx.y;
  const int og = A.octet_bits, ae = A.g.ae, ke = A.g.ke, m = A.g.m;
  const int tile = (int)blockIdx.x % A.g.n_tiles, split = (int)blockIdx.x / A.g.n_tiles;
  int p, q;
  rdmb::tile_pq(tile, p, q);
  const bool diag = p == q;
  // (a wave of the diagonal tile above the diagonal has nothing to compute)
  const bool idle = diag && 32 * wc > 16 * wr + 15;
  const int64_t len = (int64_t)1 << A.L_eff;
  const double2* st = A.state + state_base(b, len, og);
  const double2* st_p =
      st + octet_spread((int64_t)rdmb::amp_index(ae, ke, (uint64_t)p << rdmb::kPanelBits, 0), og);
  const double2* st_q =
      st + octet_spread((int64_t)rdmb::amp_index(ae, ke, (uint64_t)q << rdmb::kPanelBits, 0), og);

  // local index v = t | j << 9 of register j: every map is linear over v's bits
  const int slot_t = rdmb::lds_slot(rdmb::local_row(t, m), rdmb::local_col(t, m));
  const int64_t goff_t = octet_spread(
      (int64_t)rdmb::amp_index(ae, ke, rdmb::local_row(t, m), rdmb::local_col(t, m)), og);
  int slot_j[kGramRegs];
  int64_t goff_j[kGramRegs];
#pragma unroll
  for (int j = 0; j < kGramRegs; ++j) {
    const int r = rdmb::local_row(j << 9, m), c = rdmb::local_col(j << 9, m);
    slot_j[j] = rdmb::lds_slot(r, c);
    goff_j[j] = octet_spread((int64_t)rdmb::amp_index(ae, ke, r, c), og);
  }

  // (columns 32 wc .. and 32 wc + 16 ..)
  d4v re0 = {0.0, 0.0, 0.0, 0.0}, re1 = re0, im0 = re0, im1 = re0;

  // lane l supplies row l & 15 of its block, column 4 s + (l >> 4) of k-step s
  const int xa0 = rdmb::lds_slot(16 * wr + (lane & 15), lane >> 4);
  const int xb0 = rdmb::lds_slot(32 * wc + (lane & 15), lane >> 4);
  auto mma = [&](d4v& c0, d4v& c1) __attribute__((always_inline)) {
    if (idle) return;
    // (lds_slot is linear: the operand of k-step s sits at the lane's slot of
    // k-step 0 XOR a constant; formed here, phase by phase, not kept in 48
    // registers across the chunk loop)
    int xa = xa0, xb = xb0;
    asm volatile("" : "+v"(xa), "+v"(xb));
#pragma unroll
    for (int s = 0; s < rdmb::kChunk / 4; ++s) {
      const int cs = rdmb::lds_slot(0, 4 * s);
      const double a0 = s_a[xa ^ cs];
      const double b0 = s_b[xb ^ cs], b1 = s_b[xb ^ cs ^ 16];
      c0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, c0, 0, 0, 0);
      c1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, c1, 0, 0, 0);
    }
  };

  const int cps = A.g.n_chunks / A.g.n_split;
  for (int ch = split * cps; ch < (split + 1) * cps; ++ch) {
    const int64_t cbase = octet_spread(
        (int64_t)rdmb::amp_index(ae, ke, 0, (uint64_t)ch << rdmb::kChunkBits), og);
    d2v vp[kGramRegs], vq[kGramRegs];
#pragma unroll
    for (int j = 0; j < kGramRegs; ++j)
      vp[j] = __builtin_nontemporal_load((const d2v*)(st_p + cbase + goff_j[j] + goff_t));
    if (diag) {
#pragma unroll
      for (int j = 0; j < kGramRegs; ++j) vq[j] = vp[j];
    } else {
#pragma unroll
      for (int j = 0; j < kGramRegs; ++j)
        vq[j] = __builtin_nontemporal_load((const d2v*)(st_q + cbase + goff_j[j] + goff_t));
    }
    __syncthreads();  // the previous chunk's last reads
#pragma unroll
    for (int j = 0; j < kGramRegs; ++j) {
      s_a[slot_t ^ slot_j[j]] = vp[j].x;
      s_b[slot_t ^ slot_j[j]] = vq[j].x;
    }
    __syncthreads();
    mma(re0, re1);  // R_p R_q^T
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kGramRegs; ++j) s_a[slot_t ^ slot_j[j]] = vp[j].y;
    __syncthreads();
    mma(im0, im1);  // I_p R_q^T
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kGramRegs; ++j) s_b[slot_t ^ slot_j[j]] = vq[j].y;
    __syncthreads();
    mma(re0, re1);  // I_p I_q^T
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kGramRegs; ++j) s_a[slot_t ^ slot_j[j]] = -vp[j].x;
    __syncthreads();
    mma(im0, im1);  // (-R_p) I_q^T
  }
  if (idle) return;

  // C/D of the f64 MFMA: register r of lane l is (row (l >> 4) + 4 r, col l & 15)
  const int de = 1 << ke;
  const bool direct = A.g.n_split == 1 && A.g.n_pad == 1;
  double* dst = direct ? A.work + (int64_t)b * A.work_stride
                       : A.partial + ((int64_t)b * A.g.n_split + split) * ((int64_t)2 * de * de);
#pragma unroll
  for (int bj = 0; bj < 2; ++bj)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int R = (p << rdmb::kPanelBits) + 16 * wr + (lane >> 4) + 4 * r;
      const int C = (q << rdmb::kPanelBits) + 32 * wc + 16 * bj + (lane & 15);
      if (C > R) continue;
      const double gr = (bj ? re1 : re0)[r];
      const double gi = R == C ? 0.0 : (bj ? im1 : im0)[r];
      *(d2v*)(dst + 2 * ((int64_t)R * de + C)) = d2v{gr, gi};
      if (direct && R != C) *(d2v*)(dst + 2 * ((int64_t)C * de + R)) = d2v{gr, -gi};
    }
}

// grid (ceil(d d / 256), batch): the lower triangle of the work matrix from the
// partials, and its conjugate
__global__ __launch_bounds__(kThreads) void rdm_block_finish_kernel(RdmBlockArgs A) {
  const int d = 1 << A.g.k, de = 1 << A.g.ke;
  const int e = (int)blockIdx.x * kThreads + (int)threadIdx.x;
  const int al = e >> A.g.k, ap = e & (d - 1);
  if (al >= d || ap > al) return;
  const int b = (int)blockIdx.y;
  const double* part = A.partial + (int64_t)b * A.g.n_split * ((int64_t)2 * de * de);
  double gr = 0.0, gi = 0.0;
  for (int pi = 0; pi < A.g.n_pad; ++pi) {
    const int64_t at =
        2 * ((int64_t)rdmb::padded_row(A.g, al, pi) * de + rdmb::padded_row(A.g, ap, pi));
    for (int s = 0; s < A.g.n_split; ++s) {
      const d2v v = *(const d2v*)(part + (int64_t)s * 2 * de * de + at);
      gr += v.x;
      gi += v.y;
    }
  }
  double* out = A.work + (int64_t)b * A.work_stride;
  if (al == ap) {
    *(d2v*)(out + 2 * ((int64_t)al * d + al)) = d2v{gr, 0.0};
    return;
  }
  *(d2v*)(out + 2 * ((int64_t)al * d + ap)) = d2v{gr, gi};
  *(d2v*)(out + 2 * ((int64_t)ap * d + al)) = d2v{gr, -gi};
}

// grid (batch): purity[b * purity_stride] = sum over the work matrix of |G|^2
__global__ __launch_bounds__(kThreads) void rdm_block_purity_kernel(RdmBlockArgs A) {
  __shared__ double s_p[kThreads];
  const int t = (int)threadIdx.x, b = (int)blockIdx.x;
  const int64_t n = (int64_t)1 << (2 * A.g.k);
  const d2v* wm = (const d2v*)(A.work + (int64_t)b * A.work_stride);
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t e0 = t; e0 < n; e0 += 4 * kThreads) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t e = e0 + (int64_t)u * kThreads;
      if (e >= n) continue;
      const d2v v = wm[e];
      a[u] += v.x * v.x + v.y * v.y;
    }
  }
  s_p[t] = (a[0] + a[1]) + (a[2] + a[3]);
  __syncthreads();
  for (int h = kThreads / 2; h >= 1; h >>= 1) {
    if (t < h) s_p[t] += s_p[t + h];
    __syncthreads();
  }
  if (t == 0) A.purity[(int64_t)b * A.purity_stride] = s_p[0];
}

hipError_t launch_rdm_block_gram(const RdmBlockArgs& a, hipStream_t stream) {
  if (!rdm_block_args_ok(a) || !a.state || !a.work || !a.partial ||
      a.work_stride < ((int64_t)2 << (2 * a.g.k)))
    return hipErrorInvalidValue;
  const bool direct = a.g.n_split == 1 && a.g.n_pad == 1;
  hipLaunchKernelGGL(rdm_block_gram_kernel,
                     dim3((unsigned)(a.g.n_tiles * a.g.n_split), (unsigned)a.batch),
                     dim3(kGramThreads), 0, stream, a);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess || direct) return err;
  const int dd = 1 << (2 * a.g.k);
  hipLaunchKernelGGL(rdm_block_finish_kernel,
                     dim3((unsigned)((dd + kThreads - 1) / kThreads), (unsigned)a.batch),
                     dim3(kThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_rdm_block_purity(const RdmBlockArgs& a, hipStream_t stream) {
  if (!rdm_block_args_ok(a) || !a.work || !a.purity || a.purity_stride < 1 ||
      a.work_stride < ((int64_t)2 << (2 * a.g.k)))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(rdm_block_purity_kernel, dim3((unsigned)a.batch), dim3(kThreads), 0, stream,
                     a);
  return hipGetLastError();
}

}  // namespace dtc
