// On-device numeric assembly of the FULL Galerkin system: the element loop of
// `do_isotropic_elliptic_assembly` / `update_isotropic_elliptic_assembly!` (Fem/EllipticPde.jl:187-275 / :291-377) for a
// fixed mesh / Dirichlet maps / f / uexact and a NEW nodal coefficient vector — what the realization loops of Examples 06,
// 09, 12-17, 19 and 20 redo on the host per draw.
//
// The index half is the row-owned plan of full_assembly_plan.hpp; this file is the numeric half:
//   k_assemble_full   one workgroup per row block, one thread per row. A thread walks the incidence list of its node
//                     (ascending element). Per incidence it reads the three cell nodes, their coordinates and coefficients and
//                     forms Δa = ((a1 + a2) + a3)/3, the shoelace terms, Area = (Δx3 Δy2 - Δx2 Δy3)/2 and, for its own vertex i
//                     and j = 0, 1, 2, ΔK_ij = Δa (Δy_i Δy_j + Δx_i Δx_j)/4/Area (:315-343). ΔK_ij goes to the row's entry in the
//                     workgroup's LDS segment, or, for a Dirichlet vertex j, as -(ue_j ΔK_ij) to b[r] (j ascending), then Δb_i
//                     (:334-375). Only the owning thread touches its row; the segment leaves with coalesced plain stores.
//   k_diag_from_csr   dinv[r] = 1.0 / A[r, r]: the Jacobi M of a refreshed matrix
// Same operations in the same order as the host path (library built with -ffp-contract=off): BIT-EXACT. No atomics, no
// communication between workgroups. Every accumulator starts at -0.0, the exact additive identity (-0.0 + t == t for every
// t, signed zeros included), so the first contribution is an assignment in effect, as in `sparse(I,J,V)`: structured meshes
// store exact zeros, one per hypotenuse, and their sign is part of the result.
#pragma once
#include "assembly.hpp"
#include "full_assembly_plan.hpp"

namespace mi {

static_assert(FA_ROWS == NT || FA_ROWS % 64 == 0, "a row block is a whole number of waves");
static_assert(FA_SEG * sizeof(double) <= 64 * 1024 && FA_SEG - 1 < (int)FA_DIR, "one segment fits the LDS; positions fit 16 bits");

// Consecutive row blocks share nodes and elements: blocks b*per .. (b+1)*per - 1 run on XCD b (workgroups are dealt to the 8
// XCDs round robin), so that the gathers of neighbouring rows meet in one L2. The grid is 8 * per workgroups.
__global__ __launch_bounds__(FA_ROWS) void k_assemble_full(int nblk, int per, int nel, int n_node, const int *__restrict__ blk_row,
                                                           const int *__restrict__ rowptr, const int *__restrict__ diag_pos,
                                                           const int *__restrict__ inc_ptr, const int *__restrict__ inc_code,
                                                           const unsigned *__restrict__ inc_pos, const int *__restrict__ cells,
                                                           const double *__restrict__ points, const double *__restrict__ ue,
                                                           const double *__restrict__ be, const double *__restrict__ a,
                                                           double *__restrict__ values, double *__restrict__ b) {
  __shared__ double seg[FA_SEG];
  const int blk = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
  if (blk >= nblk) return;                     // the whole workgroup leaves: nobody waits at the barrier below
  const int row0 = blk_row[blk], row1 = blk_row[blk + 1];
  const int e0 = rowptr[row0];
  const int seg_len = rowptr[row1] - e0;       // <= FA_SEG by the plan
  const int r = row0 + (int)threadIdx.x;
  if (r < row1) {
    const int off = rowptr[r] - e0, len = rowptr[r + 1] - rowptr[r];
    for (int k = 0; k < len; ++k) seg[off + k] = -0.0;
    const unsigned dpos = (unsigned)diag_pos[r];
    const int q0 = inc_ptr[r], q1 = inc_ptr[r + 1];
    const double *__restrict__ px = points, *__restrict__ py = points + n_node;
    double acc = -0.0;
    for (int q = q0; q < q1; ++q) {
      const int code = inc_code[q];
      unsigned packed = inc_pos[q];
      const int e = code >> 2, i = code & 3;
      const int c0 = cells[e], c1 = cells[(long long)nel + e], c2 = cells[2 * (long long)nel + e];
      const double x0 = px[c0], x1 = px[c1], x2 = px[c2];
      const double y0 = py[c0], y1 = py[c1], y2 = py[c2];
      const double da = ((a[c0] + a[c1]) + a[c2]) / 3.0;
      const double dx[3] = {x2 - x1, x0 - x2, x1 - x0};
      const double dy[3] = {y1 - y2, y2 - y0, y0 - y1};
      const double area = (dx[2] * dy[1] - dx[1] * dy[2]) / 2.0;
      const double dxi = i == 0 ? dx[0] : i == 1 ? dx[1] : dx[2];
      const double dyi = i == 0 ? dy[0] : i == 1 ? dy[1] : dy[2];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double K = da * (dyi * dy[j] + dxi * dx[j]) / 4 / area;
        unsigned pos = dpos;
        if (j != i) { pos = packed & 0xFFFFu; packed >>= 16; }
        if (pos == FA_DIR) acc = acc + -(ue[(long long)j * nel + e] * K);
        else seg[off + (int)pos] = seg[off + (int)pos] + K;
      }
      acc = acc + be[(long long)i * nel + e];
    }
    b[r] = q1 > q0 ? acc : 0.0;                // a free node of no element: `b = zeros(n)` stays
  }
  __syncthreads();
  for (int k = (int)threadIdx.x; k < seg_len; k += FA_ROWS) values[(long long)e0 + k] = seg[k];
}

// mode 0: *missing = a row that stores no diagonal (any one of them), nothing else is written; mode 1: dinv[r] = 1.0 / A[r, r]
__global__ __launch_bounds__(NT) void k_diag_from_csr(int n, int mode, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                      const double *__restrict__ val, double *__restrict__ dinv, int *__restrict__ missing) {
  for (int r = blockIdx.x * NT + threadIdx.x; r < n; r += gridDim.x * NT) {
    int at = -1;
    for (int k = rowptr[r]; k < rowptr[r + 1]; ++k)
      if (col[k] == r) { at = k; break; }
    if (mode == 0) { if (at < 0) *missing = r; }
    else if (at >= 0) dinv[r] = 1.0 / val[at];
  }
}

}  // namespace mi
