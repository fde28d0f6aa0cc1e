// Host driver of csrc/spmv_blocks.hpp (the row blocks of the CSR-stream SpMV and their dealing to the XCDs).
// Usage: spmv_blocks_check FILE...   FILE: little-endian int32 words: n_rows, n_breaks, rowptr (n_rows + 1), breaks (n_breaks).
// For every file it prints one JSON line {"tile", "n", "blocks": [[r0, r1, k0, k1], ...], "xcd_row": [9 rows]}: exactly what
// CsrDev::upload hands to the kernels. The checks themselves are tests/test_sparse_edges_cpu.py's.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../julia-phd-krylov-spdes_amd/csrc/spmv_blocks.hpp"

int main(int argc, char **argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s FILE...\n", argv[0]); return 2; }
  for (int f = 1; f < argc; ++f) {
    FILE *fp = std::fopen(argv[f], "rb");
    if (!fp) { std::fprintf(stderr, "cannot open %s\n", argv[f]); return 2; }
    int32_t head[2];
    if (std::fread(head, sizeof(int32_t), 2, fp) != 2 || head[0] < 0 || head[1] < 0) return 2;
    const int n = head[0];
    std::vector<int> rowptr((size_t)n + 1), breaks((size_t)head[1]);
    if (std::fread(rowptr.data(), sizeof(int32_t), rowptr.size(), fp) != rowptr.size()) return 2;
    if (!breaks.empty() && std::fread(breaks.data(), sizeof(int32_t), breaks.size(), fp) != breaks.size()) return 2;
    std::fclose(fp);
    const std::vector<SpmvBlock> blocks = spmv_row_blocks(n, rowptr.data(), breaks.empty() ? nullptr : &breaks);
    const std::vector<int> xr = spmv_xcd_rows(blocks, n);
    std::printf("{\"tile\": %d, \"n\": %d, \"blocks\": [", SPMV_TILE, n);
    for (size_t b = 0; b < blocks.size(); ++b)
      std::printf("%s[%d, %d, %d, %d]", b ? ", " : "", blocks[b].r0, blocks[b].r1, blocks[b].k0, blocks[b].k1);
    std::printf("], \"xcd_row\": [");
    for (size_t x = 0; x < xr.size(); ++x) std::printf("%s%d", x ? ", " : "", xr[x]);
    std::printf("]}\n");
  }
  return 0;
}
