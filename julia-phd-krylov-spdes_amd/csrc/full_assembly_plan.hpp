// Host half of the full-system assembly (full_assembly.hpp): the index plan of `do_isotropic_elliptic_assembly` /
// `update_isotropic_elliptic_assembly!` (Fem/EllipticPde.jl:187-275 / :291-377) for a fixed mesh and fixed Dirichlet maps.
// Host only, no HIP, so that a CPU test compiles it (tests/cpp/full_assembly_plan_check.cpp). `fem.make_full_assembly_plan` is
// its python mirror: same arrays, same names.
//
// The plan is ROW-OWNED: free node r is row r of A, and everything that lands in row r and in b[r] comes from the elements
// incident to that node, visited in ascending element number — the order in which `sparse(I,J,V)` and `b[k] +=` combine
// their contributions. From (cells, points, point_marker) the plan holds
//   node_row[n_node]     row of a node, -1 on a Dirichlet node (point_marker == 1); free nodes are numbered ascending
//   rowptr, colidx       CSR pattern of A, sorted rows (A is bitwise symmetric: these are also its CSC arrays)
//   diag_pos[n]          position of the diagonal entry inside its row
//   inc_ptr[n + 1]       incidence list of every row ...
//   inc_code[ninc]       ... 4 e + i: element e has the row's node as its local vertex i; ascending e
//   inc_pos[ninc]        for the two OTHER vertices of e, ascending local index: low / high 16 bits = position in the row of
//                        that vertex's column, or FA_DIR: a Dirichlet vertex, whose pair feeds b[r] as a lifting term
//   blk_row[nblk + 1]    row blocks: at most FA_ROWS consecutive rows (one thread each), at most FA_SEG stored entries (one
//                        workgroup's LDS segment), never a split row
// Nothing of size 9 nel: the kernel recomputes the geometry from `points`.
// Refusals (BAD_ARG, `err` names the numbers): a cell index outside [0, n_node) after the base shift, an element with a
// repeated vertex, a zero-area element, a row longer than FA_SEG, 4 nel >= 2^31, a pattern that is not the mesh's.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace mi {

constexpr int FA_ROWS = 256;        // rows per workgroup = threads per workgroup
constexpr int FA_SEG = 4096;        // stored entries per workgroup: 32 KiB of LDS
constexpr unsigned FA_DIR = 0xFFFF;  // "Dirichlet" in a 16-bit row position (FA_SEG - 1 < FA_DIR)

namespace fap {

struct Plan {
  int nel = 0, n_node = 0, n = 0;
  std::vector<int> cells;                          // (3, nel), 0-based
  std::vector<int> node_row, rowptr, colidx, diag_pos, inc_ptr, inc_code, blk_row;
  std::vector<unsigned> inc_pos;
  int64_t nnz() const { return (int64_t)colidx.size(); }
  int64_t ninc() const { return (int64_t)inc_code.size(); }
  int nblk() const { return (int)blk_row.size() - 1; }
  // what the device keeps of the plan: the index arrays, ue and be (3 nel each) and the points (2 n_node)
  int64_t bytes() const {
    return 4 * (int64_t)(cells.size() + rowptr.size() + diag_pos.size() + inc_ptr.size() + inc_code.size() + inc_pos.size() + blk_row.size()) +
           8 * (6 * (int64_t)nel + 2 * (int64_t)n_node);
  }
};

enum Status { OK = 0, BAD_ARG = 1 };

inline int refuse(std::string &err, const char *fmt, long long a = 0, long long b = 0, long long c = 0) {
  char buf[256];
  std::snprintf(buf, sizeof buf, fmt, a, b, c);
  err = buf;
  return BAD_ARG;
}

// Area of element e in the operation order of EllipticPde.jl:319-327 (fem._element_geometry)
inline double element_area(const double *points, int64_t n_node, int c0, int c1, int c2) {
  const double *x = points, *y = points + n_node;
  const double dx1 = x[c0] - x[c2], dx2 = x[c1] - x[c0];
  const double dy1 = y[c2] - y[c0], dy2 = y[c0] - y[c1];
  return (dx2 * dy1 - dx1 * dy2) / 2.0;
}

// cells: (3, nel) row-major, entries shifted by index_base; points: (2, n_node) row-major; point_marker[n_node]: 1 = Dirichlet.
// rowptr / colidx (entries shifted by index_base, n rows): the pattern the caller holds; both NULL: nothing to compare with.
inline int make_plan(int64_t nel, int64_t n_node, const int64_t *cells, int index_base, const double *points, const int64_t *point_marker,
                     int64_t n, const int64_t *rowptr, const int64_t *colidx, Plan &pl, std::string &err) {
  pl = Plan();
  if (nel < 1) return refuse(err, "full assembly plan: nel = %lld elements (at least 1 expected)", (long long)nel);
  if (4 * nel >= ((int64_t)1 << 31)) return refuse(err, "full assembly plan: nel = %lld elements: 4 nel = %lld does not fit 31 bits", (long long)nel, (long long)(4 * nel));
  if (n_node < 1 || n_node >= ((int64_t)1 << 31)) return refuse(err, "full assembly plan: n_node = %lld nodes (1 <= n_node < 2^31 expected)", (long long)n_node);
  if (!cells || !points || !point_marker) return refuse(err, "full assembly plan: cells, points or point_marker is NULL");
  if (index_base != 0 && index_base != 1) return refuse(err, "full assembly plan: index_base = %lld is neither 0 nor 1", index_base);
  if ((rowptr == nullptr) != (colidx == nullptr)) return refuse(err, "full assembly plan: one of rowptr and colidx is NULL, the other is not");
  pl.nel = (int)nel; pl.n_node = (int)n_node;
  pl.cells.resize((size_t)3 * nel);
  for (int64_t e = 0; e < nel; ++e) {
    int c[3];
    for (int i = 0; i < 3; ++i) {
      const int64_t v = cells[(size_t)i * nel + e] - index_base;
      if (v < 0 || v >= n_node)
        return refuse(err, "full assembly plan: element %lld, vertex %lld: node %lld is outside the mesh", (long long)(e + index_base), (long long)i, (long long)cells[(size_t)i * nel + e]);
      c[i] = (int)v;
      pl.cells[(size_t)i * nel + e] = c[i];
    }
    if (c[0] == c[1] || c[1] == c[2] || c[0] == c[2])
      return refuse(err, "full assembly plan: element %lld lists node %lld twice", (long long)(e + index_base), (long long)((c[0] == c[1] || c[0] == c[2] ? c[0] : c[1]) + index_base));
    const double area = element_area(points, n_node, c[0], c[1], c[2]);
    if (!(area != 0.0) || !(area - area == 0.0))
      return refuse(err, "full assembly plan: element %lld has zero area (or coordinates that are not finite)", (long long)(e + index_base));
  }
  // rows: the free nodes, ascending (get_dirichlet_inds, Fem/BoundaryConditions.jl:35-57)
  pl.node_row.assign((size_t)n_node, -1);
  int nfree = 0;
  for (int64_t v = 0; v < n_node; ++v)
    if (point_marker[v] != 1) pl.node_row[(size_t)v] = nfree++;
  if (rowptr && n != nfree)
    return refuse(err, "full assembly plan: the pattern has n = %lld rows, the mesh has %lld free nodes", (long long)n, (long long)nfree);
  pl.n = nfree;
  // incidence lists, ascending element
  pl.inc_ptr.assign((size_t)nfree + 1, 0);
  for (int64_t k = 0; k < 3 * nel; ++k) {
    const int r = pl.node_row[(size_t)pl.cells[(size_t)k]];
    if (r >= 0) pl.inc_ptr[(size_t)r + 1]++;
  }
  for (int r = 0; r < nfree; ++r) pl.inc_ptr[(size_t)r + 1] += pl.inc_ptr[(size_t)r];
  const size_t ninc = (size_t)pl.inc_ptr[(size_t)nfree];
  pl.inc_code.assign(ninc, 0);
  pl.inc_pos.assign(ninc, 0);
  {
    std::vector<int> next(pl.inc_ptr.begin(), pl.inc_ptr.end() - 1);
    for (int64_t e = 0; e < nel; ++e)
      for (int i = 0; i < 3; ++i) {
        const int r = pl.node_row[(size_t)pl.cells[(size_t)i * nel + e]];
        if (r >= 0) pl.inc_code[(size_t)next[(size_t)r]++] = (int)(4 * e + i);
      }
  }
  // pattern: row r holds the free vertices of its incident elements
  pl.rowptr.assign((size_t)nfree + 1, 0);
  pl.diag_pos.assign((size_t)nfree, 0);
  std::vector<int> cols;
  for (int r = 0; r < nfree; ++r) {
    cols.clear();
    for (int q = pl.inc_ptr[(size_t)r]; q < pl.inc_ptr[(size_t)r + 1]; ++q) {
      const int e = pl.inc_code[(size_t)q] >> 2;
      for (int j = 0; j < 3; ++j) {
        const int c = pl.node_row[(size_t)pl.cells[(size_t)j * nel + e]];
        if (c >= 0) cols.push_back(c);
      }
    }
    std::sort(cols.begin(), cols.end());
    cols.erase(std::unique(cols.begin(), cols.end()), cols.end());
    if ((int64_t)cols.size() > FA_SEG)
      return refuse(err, "full assembly plan: row %lld has %lld stored entries, more than FA_SEG = %lld", (long long)(r + index_base), (long long)cols.size(), (long long)FA_SEG);
    if ((int64_t)pl.colidx.size() + (int64_t)cols.size() >= INT32_MAX)
      return refuse(err, "full assembly plan: more than 2^31 - 2 stored entries up to row %lld", (long long)(r + index_base));
    pl.diag_pos[(size_t)r] = (int)(std::lower_bound(cols.begin(), cols.end(), r) - cols.begin());
    pl.colidx.insert(pl.colidx.end(), cols.begin(), cols.end());
    pl.rowptr[(size_t)r + 1] = (int)pl.colidx.size();
  }
  if (rowptr) {
    for (int r = 0; r <= nfree; ++r)
      if (rowptr[r] - index_base != pl.rowptr[(size_t)r])
        return refuse(err, "full assembly plan: rowptr[%lld] = %lld, the mesh gives %lld", (long long)r, (long long)rowptr[r], (long long)pl.rowptr[(size_t)r] + index_base);
    for (size_t k = 0; k < pl.colidx.size(); ++k)
      if (colidx[k] - index_base != pl.colidx[k])
        return refuse(err, "full assembly plan: colidx[%lld] = %lld, the mesh gives %lld", (long long)k, (long long)colidx[k], (long long)pl.colidx[k] + index_base);
  }
  // positions of the other two vertices' columns in the row
  for (int r = 0; r < nfree; ++r) {
    const int *row = pl.colidx.data() + pl.rowptr[(size_t)r];
    const int len = pl.rowptr[(size_t)r + 1] - pl.rowptr[(size_t)r];
    for (int q = pl.inc_ptr[(size_t)r]; q < pl.inc_ptr[(size_t)r + 1]; ++q) {
      const int e = pl.inc_code[(size_t)q] >> 2, i = pl.inc_code[(size_t)q] & 3;
      unsigned packed = 0;
      int slot = 0;
      for (int j = 0; j < 3; ++j) {
        if (j == i) continue;
        const int c = pl.node_row[(size_t)pl.cells[(size_t)j * nel + e]];
        const unsigned pos = c < 0 ? FA_DIR : (unsigned)(std::lower_bound(row, row + len, c) - row);
        packed |= pos << (16 * slot++);
      }
      pl.inc_pos[(size_t)q] = packed;
    }
  }
  // row blocks
  pl.blk_row.push_back(0);
  int r0 = 0;
  for (int r = 0; r < nfree; ++r)
    if (r - r0 == FA_ROWS || pl.rowptr[(size_t)r + 1] - pl.rowptr[(size_t)r0] > FA_SEG) {
      pl.blk_row.push_back(r);
      r0 = r;
    }
  if (nfree) pl.blk_row.push_back(nfree);
  err.clear();
  return OK;
}

}  // namespace fap
}  // namespace mi
