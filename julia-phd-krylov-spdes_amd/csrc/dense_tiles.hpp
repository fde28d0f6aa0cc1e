// Tile list of the dense-block operators (operators.hpp: DenseBlockOp; kernels.hpp: k_gemv_batched, k_gemv_pcg) and the
// tiling a rank chooses for a slice of the blocks.
// Host code without HIP: the library (DenseBlockOp's constructor) and the host check tests/cpp/dense_tiles_check.cpp
// compile the same list.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

struct GemvTile {
  long long mat_off;  // element offset of the subdomain block
  int n, ld;          // n_Γd and padded leading dimension
  int loc_off, row0;  // offset of the block in the local index space, first row of this tile
  int active, nrows;  // active 0: the block of this subdomain lives on another rank (multi-GPU): nothing to stream here;
                      // otherwise 1 + the slot of this tile's partial dot products in the folded launches.
                      // nrows: rows [row0, row0 + nrows) whose owner duties this tile performs in the folded launches
                      // (active: the WAVES*RPW streamed rows; inactive: up to one row per thread)
};
constexpr int GEMV_PANEL = 2048;  // doubles of x_d staged per pass (16 KiB LDS)
constexpr int PART_ROWS = 4;      // fewest rows a streamed tile can have (4 waves x 1 row)

struct DenseTiling {
  int waves, rpw;  // waves per workgroup (4, 8 or 16), rows per wave (1, 2 or 4)
};

// A rank that owns 1/N of the blocks would keep 1/N of the CUs busy with 32-row tiles (a launch lasts as long as
// one tile): cut the owned rows into about one tile per CU instead.
inline DenseTiling dense_sharded_tiling(int64_t owned_rows, int n_cu) {
  const int64_t per_tile = std::max<int64_t>(1, owned_rows / std::max(1, n_cu));
  if (per_tile >= 24) return DenseTiling{16, 2};
  if (per_tile >= 12) return DenseTiling{16, 1};
  if (per_tile >= 6) return DenseTiling{8, 1};
  return DenseTiling{4, 1};
}

struct DenseTilePlan {
  std::vector<GemvTile> tiles;
  std::vector<long long> moff;  // per local subdomain: element offset of its block (0 for a block stored elsewhere)
  std::vector<int> ld;          // per local subdomain: padded row stride
  int part_total = 0;           // slots of one partial-dot array
  int max_nd = 0, max_ld = 0;
  long long elems = 0;          // elements of the owned blocks, padded
};

// nd / loc_off: rows and local offset of every subdomain of the maps; [own0, own1): the ones whose blocks are stored here.
// sharded_parts: the partial-dot slots follow the layout every rank derives from the maps alone (below).
// line: elements per 128-byte line (16 doubles / 32 floats).
inline DenseTilePlan dense_tile_plan(const std::vector<int> &nd, const std::vector<int> &loc_off, int own0, int own1,
                                     DenseTiling tiling, bool sharded_parts, int line) {
  DenseTilePlan p;
  const int waves = tiling.waves, rpw = tiling.rpw;
  long long tot = 0;
  for (int dl = 0; dl < (int)nd.size(); ++dl) {
    const int n_d = nd[dl];
    // rows padded to whole 128-byte lines
    int l = (n_d + line - 1) / line * line;
    // A row stride that is a multiple of 2 KiB puts every row of a tile on the same HBM channels: measured 27 % slower
    // at n_Γd = 1024 (profiles/r01_gemv_variant_sweep.txt). One extra 128-byte line per row breaks the pattern. The
    // pattern is one of bytes: 256 doubles, 512 floats. (l == GEMV_PANEL keeps its stride in both formats: the operand
    // panel of the folded launches holds no more columns.)
    if (l % (16 * line) == 0 && l != GEMV_PANEL) l += line;
    const bool own = dl >= own0 && dl < own1;
    p.moff.push_back(own ? tot : 0); p.ld.push_back(l);
    p.max_nd = std::max(p.max_nd, n_d);
    p.max_ld = std::max(p.max_ld, l);
    // tiles of another rank's block only do owner duties in the folded launches: as few workgroups as possible
    const int step = own ? waves * rpw : 64 * waves;
    // `active` of a streamed tile = 1 + the slot of its partial dot products. One GPU: the tile number. Sharded over ranks:
    // a layout every rank derives from the maps alone, whatever tiling each rank chose for its own blocks — subdomain
    // after subdomain, one slot per PART_ROWS rows (no tiling has fewer rows per tile), so the ranks' arrays are a
    // disjoint union of one array and the exchange adds nothing.
    for (int r = 0; r < n_d; r += step) {
      const int slot = sharded_parts ? p.part_total + r / PART_ROWS : (int)p.tiles.size();
      p.tiles.push_back(GemvTile{own ? tot : 0, n_d, l, loc_off[dl], r, own ? slot + 1 : 0, std::min(step, n_d - r)});
    }
    if (sharded_parts) p.part_total += (n_d + PART_ROWS - 1) / PART_ROWS;
    if (own) tot += (long long)n_d * l;
  }
  if (!sharded_parts) p.part_total = (int)p.tiles.size();
  p.elems = tot;
  return p;
}
