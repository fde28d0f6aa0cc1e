// Row blocks of the CSR-stream SpMV (kernels.hpp: k_spmv_csr, k_spmv_pcg, k_icg_spmv) and their dealing to the XCDs.
// Host code without HIP: the library (CsrDev::upload, InteriorCg::build_fold) and the host check
// tests/cpp/spmv_blocks_check.cpp compile the same partition.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

#ifndef MI355_SPMV_TILE
#define MI355_SPMV_TILE 1024   // 512..4096 swept on MI355X at 250k DoF: 1024 gives the shortest launch (profiles/)
#endif
constexpr int SPMV_TILE = MI355_SPMV_TILE;

struct SpmvBlock {  // one record per row block: rows [r0, r1), non-zeros [k0, k1)
  int r0, r1, k0, k1;
};

// Greedy row blocks of <= SPMV_TILE non-zeros (a longer row stands alone). A block prefers to start at
// an even non-zero offset (paired loads in the kernel): if the greedy end lands on an odd offset, give
// back up to three rows to reach an even one.
// `rowptr` holds n_rows + 1 offsets. `breaks` (ascending row indices): a row block never crosses one of them
// (per-subdomain partial sums).
inline std::vector<SpmvBlock> spmv_row_blocks(int n_rows, const int *rowptr, const std::vector<int> *breaks = nullptr) {
  std::vector<SpmvBlock> blocks;
  int r = 0;
  size_t nb = 0;
  while (r < n_rows) {
    while (breaks && nb < breaks->size() && (*breaks)[nb] <= r) ++nb;
    const int limit = (breaks && nb < breaks->size()) ? std::min((*breaks)[nb], n_rows) : n_rows;
    int e = r + 1;
    while (e < limit && rowptr[e + 1] - rowptr[r] <= SPMV_TILE) ++e;
    if (e < limit && (rowptr[e] & 1))
      for (int back = 1; back <= 3 && e - back > r; ++back)
        if ((rowptr[e - back] & 1) == 0) { e -= back; break; }
    blocks.push_back(SpmvBlock{r, e, rowptr[r], rowptr[e]});
    r = e;
  }
  return blocks;
}

// [9] first row of the row blocks that run on XCD x; [8] = n_rows, as is [x] of an XCD without blocks
// (k_spmv_csr deals block b = (blockIdx & 7) * per + (blockIdx >> 3), per = ceil(nblocks / 8))
inline std::vector<int> spmv_xcd_rows(const std::vector<SpmvBlock> &blocks, int n_rows) {
  const int nblocks = (int)blocks.size();
  const int per = (nblocks + 7) >> 3;
  std::vector<int> xr(9, n_rows);
  for (int x = 0; x < 8; ++x) xr[x] = x * per < nblocks ? blocks[(size_t)x * per].r0 : n_rows;
  return xr;
}
