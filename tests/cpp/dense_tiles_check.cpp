// Host driver of csrc/dense_tiles.hpp (the tile list of the dense-block operators and the tiling a rank chooses for its slice).
// Usage: dense_tiles_check FILE...   FILE: whitespace-separated integers:
//   ndom world n_cu line sharded_parts, then ndom block sizes, then per rank: lo hi waves rpw (waves 0: the automatic rule).
// The maps are those of ALL subdomains (what a sharded operator is built on), the owned blocks of rank r are [lo, hi).
// For every file it prints one JSON line {"ranks": [{"waves", "rpw", "part_total", "max_nd", "max_ld", "elems", "moff": [...],
// "ld": [...], "tiles": [[mat_off, n, ld, loc_off, row0, active, nrows], ...]}, ...]}: exactly what DenseBlockOp's constructor
// hands to the kernels. The checks themselves are tests/test_shard_edges_cpu.py's.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../julia-phd-krylov-spdes_amd/csrc/dense_tiles.hpp"

int main(int argc, char **argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s FILE...\n", argv[0]); return 2; }
  for (int f = 1; f < argc; ++f) {
    FILE *fp = std::fopen(argv[f], "r");
    if (!fp) { std::fprintf(stderr, "cannot open %s\n", argv[f]); return 2; }
    int ndom, world, n_cu, line, sharded;
    if (std::fscanf(fp, "%d %d %d %d %d", &ndom, &world, &n_cu, &line, &sharded) != 5 || ndom < 0 || world < 1) return 2;
    std::vector<int> nd((size_t)ndom), loc_off((size_t)ndom);
    long long tot = 0;
    for (int d = 0; d < ndom; ++d) {
      if (std::fscanf(fp, "%d", &nd[d]) != 1 || nd[d] < 0) return 2;
      loc_off[d] = (int)tot;
      tot += nd[d];
    }
    std::printf("{\"ranks\": [");
    for (int r = 0; r < world; ++r) {
      int lo, hi, waves, rpw;
      if (std::fscanf(fp, "%d %d %d %d", &lo, &hi, &waves, &rpw) != 4 || lo < 0 || hi > ndom || lo > hi) return 2;
      DenseTiling tl{waves, rpw};
      if (waves == 0) {
        int64_t owned_rows = 0;
        for (int d = lo; d < hi; ++d) owned_rows += nd[d];
        tl = dense_sharded_tiling(owned_rows, n_cu);
      }
      const DenseTilePlan p = dense_tile_plan(nd, loc_off, lo, hi, tl, sharded != 0, line);
      std::printf("%s{\"waves\": %d, \"rpw\": %d, \"part_total\": %d, \"max_nd\": %d, \"max_ld\": %d, \"elems\": %lld, \"moff\": [", r ? ", " : "",
                  tl.waves, tl.rpw, p.part_total, p.max_nd, p.max_ld, p.elems);
      for (size_t d = 0; d < p.moff.size(); ++d) std::printf("%s%lld", d ? ", " : "", p.moff[d]);
      std::printf("], \"ld\": [");
      for (size_t d = 0; d < p.ld.size(); ++d) std::printf("%s%d", d ? ", " : "", p.ld[d]);
      std::printf("], \"tiles\": [");
      for (size_t t = 0; t < p.tiles.size(); ++t) {
        const GemvTile &g = p.tiles[t];
        std::printf("%s[%lld, %d, %d, %d, %d, %d, %d]", t ? ", " : "", g.mat_off, g.n, g.ld, g.loc_off, g.row0, g.active, g.nrows);
      }
      std::printf("]}");
    }
    std::printf("]}\n");
    std::fclose(fp);
  }
  return 0;
}
