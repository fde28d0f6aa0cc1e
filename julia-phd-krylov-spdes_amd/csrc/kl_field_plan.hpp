// Host half of the realization sampler (kl_field.hpp): the tiling of its launches and the index plan of the factored draw.
// Host only, no HIP, so that a CPU test compiles it (tests/cpp/kl_field_plan_check.cpp).
//
// Tiling (klf_tiling): a pure function of (n, m, nreal), like cov_tiling. One thread owns one node and up to KLF_RB
// realization accumulators; a workgroup owns KLF_ROW_TILE nodes; the coefficients c[α, r] = sqrt(Λ_α) Ξ[α, r] go through LDS
// in chunks of KLF_MODE_CHUNK modes. The mode sum of a node is never split. Only the column sums of get_kl_coordinates are:
// the row tiles are dealt to `coord_splits` workgroups per block of KLF_RB columns, whole tiles per split, as many splits as
// bring the launch to about 4 KLF_FILL workgroups (at most KLF_MAX_SPLITS, at most one per tile).
//
// Factored draw (make_dd_plan), `draw(mesh, Λ, Φ, Φd, inds_l2gd)` of Fem/KarhunenLoeveDomainDecomposition.jl:850-883 with
// g_i = (1 / cnt_i) Σ_{d ∋ i} Σ_α Φd[d][l, α] y[off_d + α],  y = Φ c. From the subdomain sizes n_d, the local mode counts md_d
// and the concatenated local-to-global maps the plan holds
//   y_off[d], t_off[d], phid_off[d]   prefix sums of md_d, n_d and n_d md_d: where subdomain d starts in y, in the local
//                                     results t and in the concatenated column-major blocks Φd
//   tiles      (d, first local row): one workgroup each, KLF_ROW_TILE rows of one subdomain at most
//   own_ptr / own_pos   node -> the positions t_off[d] + l of its copies, ascending d: the order the gather sums in;
//                       cnt_i = own_ptr[i + 1] - own_ptr[i]
// Refusals (BAD_ARG, `err` names the numbers): sizes below 1 or above 2^30, md_d < 1, n_d < 1, an index outside [0, n) after
// the base shift, a node repeated within one subdomain, a node owned by no subdomain (the reference would divide by cnt = 0),
// more than 2^31 - 2 local rows or reduced rows in all.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace mi {

constexpr int KLF_ROW_TILE = 256;     // nodes per workgroup = threads per workgroup
constexpr int KLF_MODE_CHUNK = 64;    // modes whose coefficients are staged in LDS at a time
constexpr int KLF_RB = 8;             // realization accumulators per thread
constexpr int KLF_UNROLL = 8;         // modes whose loads are issued together (the adds stay in order)
constexpr int KLF_FILL = 256;         // workgroups that fill the grid (one per CU)
constexpr int KLF_MAX_SPLITS = 1024;  // most row splits of the coordinates launch (its workspace is coord_splits x m)
constexpr int64_t KLF_COORD_MAX_M = 65535 * (int64_t)KLF_RB;   // the coordinates launch has one grid row per block of KLF_RB modes
constexpr int64_t KLF_MAX_N = (int64_t)1 << 30;

struct KlfTiling {
  int row_tiles, real_blocks, coord_col_blocks, coord_splits, coord_tiles_per_split;
};
inline KlfTiling klf_tiling(int64_t n, int64_t m, int64_t nreal) {
  KlfTiling t;
  t.row_tiles = (int)((n + KLF_ROW_TILE - 1) / KLF_ROW_TILE);
  t.real_blocks = (int)((nreal + KLF_RB - 1) / KLF_RB);
  t.coord_col_blocks = (int)((m + KLF_RB - 1) / KLF_RB);
  int64_t want = (4 * (int64_t)KLF_FILL + t.coord_col_blocks - 1) / t.coord_col_blocks;
  want = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, t.row_tiles), KLF_MAX_SPLITS));
  t.coord_tiles_per_split = (int)((t.row_tiles + want - 1) / want);
  t.coord_splits = (t.row_tiles + t.coord_tiles_per_split - 1) / t.coord_tiles_per_split;
  return t;
}
// accumulators a launch of `nreal <= KLF_RB` realizations instantiates: 1, 2, 4 or KLF_RB
inline int klf_rb_in_use(int nreal) { return nreal > 4 ? KLF_RB : nreal > 2 ? 4 : nreal; }

namespace klfp {

struct Tile {
  int d, row0;
};
struct Plan {
  int n = 0, ndom = 0;
  int nloc = 0, nred = 0;                       // Σ n_d, Σ md_d
  std::vector<int> n_d, md, y_off, t_off;        // y_off, t_off: ndom + 1 entries
  std::vector<long long> phid_off;               // ndom + 1 entries
  std::vector<Tile> tiles;
  std::vector<int> own_ptr, own_pos;             // n + 1, nloc
  int cnt_max = 0, md_max = 0;
  // what the device keeps of the plan (the factors Φd and Φ are counted by the caller)
  int64_t bytes() const {
    return 4 * (int64_t)(n_d.size() + md.size() + y_off.size() + t_off.size() + 2 * tiles.size() + own_ptr.size() + own_pos.size()) +
           8 * (int64_t)phid_off.size();
  }
};

enum Status { OK = 0, BAD_ARG = 1 };

inline int refuse(std::string &err, const char *fmt, long long a = 0, long long b = 0, long long c = 0) {
  char buf[256];
  std::snprintf(buf, sizeof buf, fmt, a, b, c);
  err = buf;
  return BAD_ARG;
}

// `inds` is the concatenation of the ndom maps (n_d[d] entries each); nothing beyond Σ n_d entries is read, and nothing at
// all before every n_d has been checked.
inline int make_dd_plan(int64_t n, int64_t ndom, const int64_t *n_d, const int64_t *md, const int64_t *inds, int index_base, Plan &pl,
                        std::string &err) {
  pl = Plan();
  if (n < 1 || n > KLF_MAX_N) return refuse(err, "kl field plan: n = %lld nodes (1 <= n <= 2^30 expected)", (long long)n);
  if (ndom < 1 || ndom > KLF_MAX_N) return refuse(err, "kl field plan: ndom = %lld subdomains (1 <= ndom <= 2^30 expected)", (long long)ndom);
  if (!n_d || !md || !inds) return refuse(err, "kl field plan: n_d, md or inds_l2gd is NULL");
  if (index_base != 0 && index_base != 1) return refuse(err, "kl field plan: index_base = %lld is neither 0 nor 1", index_base);
  int64_t nloc = 0, nred = 0;
  for (int64_t d = 0; d < ndom; ++d) {
    if (md[d] < 1 || md[d] > KLF_MAX_N) return refuse(err, "kl field plan: md[%lld] = %lld local modes (at least 1 expected)", (long long)d, (long long)md[d]);
    if (n_d[d] < 1 || n_d[d] > n) return refuse(err, "kl field plan: n_d[%lld] = %lld nodes (1 <= n_d <= n = %lld)", (long long)d, (long long)n_d[d], (long long)n);
    nloc += n_d[d];
    nred += md[d];
    if (nloc > INT32_MAX - 1 || nred > INT32_MAX - 1)
      return refuse(err, "kl field plan: more than 2^31 - 2 local rows (%lld) or reduced rows (%lld) up to subdomain %lld", (long long)nloc, (long long)nred, (long long)d);
  }
  pl.n = (int)n; pl.ndom = (int)ndom; pl.nloc = (int)nloc; pl.nred = (int)nred;
  pl.n_d.resize((size_t)ndom); pl.md.resize((size_t)ndom);
  pl.y_off.assign((size_t)ndom + 1, 0); pl.t_off.assign((size_t)ndom + 1, 0); pl.phid_off.assign((size_t)ndom + 1, 0);
  pl.own_ptr.assign((size_t)n + 1, 0);
  std::vector<int> seen((size_t)n, -1);          // last subdomain that listed the node
  int64_t p = 0;
  for (int64_t d = 0; d < ndom; ++d) {
    pl.n_d[(size_t)d] = (int)n_d[d]; pl.md[(size_t)d] = (int)md[d];
    pl.md_max = std::max(pl.md_max, (int)md[d]);
    pl.y_off[(size_t)d + 1] = pl.y_off[(size_t)d] + (int)md[d];
    pl.t_off[(size_t)d + 1] = pl.t_off[(size_t)d] + (int)n_d[d];
    pl.phid_off[(size_t)d + 1] = pl.phid_off[(size_t)d] + (long long)n_d[d] * (long long)md[d];
    for (int64_t l = 0; l < n_d[d]; ++l, ++p) {
      const int64_t i = inds[p] - index_base;
      if (i < 0 || i >= n)
        return refuse(err, "kl field plan: inds_l2gd of subdomain %lld, entry %lld: node %lld is outside the mesh", (long long)d, (long long)l, (long long)inds[p]);
      if (seen[(size_t)i] == (int)d)
        return refuse(err, "kl field plan: subdomain %lld lists node %lld twice (second time at entry %lld)", (long long)d, (long long)inds[p], (long long)l);
      seen[(size_t)i] = (int)d;
      pl.own_ptr[(size_t)i + 1]++;
    }
    for (int64_t r0 = 0; r0 < n_d[d]; r0 += KLF_ROW_TILE) pl.tiles.push_back(Tile{(int)d, (int)r0});
  }
  for (int64_t i = 0; i < n; ++i) {
    if (pl.own_ptr[(size_t)i + 1] == 0)
      return refuse(err, "kl field plan: node %lld belongs to no subdomain (the reference would divide by cnt = 0)", (long long)(i + index_base));
    pl.cnt_max = std::max(pl.cnt_max, pl.own_ptr[(size_t)i + 1]);
    pl.own_ptr[(size_t)i + 1] += pl.own_ptr[(size_t)i];
  }
  // subdomains ascending, so every node's positions come out in ascending d
  pl.own_pos.assign((size_t)nloc, 0);
  std::vector<int> next(pl.own_ptr.begin(), pl.own_ptr.end() - 1);
  p = 0;
  for (int64_t d = 0; d < ndom; ++d)
    for (int64_t l = 0; l < n_d[d]; ++l, ++p) pl.own_pos[(size_t)next[(size_t)(inds[p] - index_base)]++] = (int)p;
  err.clear();
  return OK;
}

}  // namespace klfp
}  // namespace mi
