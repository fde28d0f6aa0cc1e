// Symbolic phase of the sparse direct `M \ r` (spd_direct.hpp): host only, no HIP, so that a CPU test compiles it
// (tests/cpp/spd_direct_check.cpp).
//
// One level of nested dissection for a sparse SPD matrix whose graph is interface-like (the A_ΓΓ of a box or mesh
// partition: 1-D chains of interface nodes that meet at cross points):
//   1. every connected component is cut into PIECES of at most P nodes, grown breadth-first from the lowest unassigned
//      node (neighbours in ascending order);
//   2. an endpoint of every edge that joins two different pieces moves into the separator Σ: a greedy vertex cover that
//      repeatedly takes the node with the most remaining cross edges (ties: lowest index). Emptied pieces are dropped;
//   3. unknowns are ordered pieces first, then Σ. With D = blockdiag(A_ii), B = A_Σ,pieces and s = A_ΣΣ - B D^-1 B':
//        y = D^-1 r_P,   z_Σ = s^-1 (r_Σ - B y),   z_P = y - D^-1 B' z_Σ.
// The numeric phase needs, per piece i, its nodes, Σ_i (the Σ nodes adjacent to piece i, ascending) and where every stored
// entry of A goes in the dense work buffer [D_i blocks | B_i' blocks (n_i x |Σ_i|) | A_ΣΣ], all column-major.
// |Σ| above `sigma_max` is refused: s^-1 is a dense |Σ| x |Σ| matrix. Recursive dissection is out of scope.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <set>
#include <string>
#include <utility>
#include <vector>

namespace mi {
namespace spd {

constexpr int SIGMA_MAX = 2048;   // largest separator: s^-1 is 32 MB
constexpr int P_DEFAULT = 64;     // piece size: a 64 x 64 fp64 block is 32 KB of LDS (DESIGN.md "Sparse direct M")
constexpr int P_MAX = 128;

struct Plan {
  int n = 0, P = 0;
  int64_t nnz = 0;
  std::vector<int> piece_of;                  // node -> piece, or -1 (Σ)
  std::vector<int> piece_ptr, piece_node;     // piece i: nodes piece_node[piece_ptr[i] .. piece_ptr[i+1]), ascending
  std::vector<int> local;                     // node -> row inside its piece, or its Σ index
  std::vector<int> sigma;                     // Σ index -> node, ascending
  std::vector<int> sig_ptr, sig_idx;          // Σ_i = sig_idx[sig_ptr[i] .. sig_ptr[i+1]) (Σ indices, ascending); slot q = position
  std::vector<int> slot_ptr, slot;            // Σ node a: its slots slot[slot_ptr[a] .. slot_ptr[a+1]), ascending (= by piece)
  std::vector<int> slot_piece;                // slot -> piece
  std::vector<int> orphan;                    // Σ nodes adjacent to no piece (written by the extra workgroup of the apply)
  std::vector<int64_t> d_off, b_off, s_off;   // per piece: offset of D_i (n_i^2), of B_i' (n_i |Σ_i|), of its |Σ_i|^2 patch
  int64_t d_total = 0, b_total = 0, patch_total = 0;
  std::vector<int64_t> dst;                   // stored entry k of A -> position in the work buffer, -1: not used (a B entry
                                              // in a Σ row; its mirror in the piece row is used)
  int n_pieces() const { return (int)piece_ptr.size() - 1; }
  int n_sigma() const { return (int)sigma.size(); }
  int64_t work_total() const { return d_total + b_total + (int64_t)n_sigma() * n_sigma(); }
};

enum Status { OK = 0, BAD_PATTERN = 1, SIGMA_TOO_LARGE = 2 };

// colptr (n + 1) / rowval (nnz) of a CSC matrix, 0-based. A structurally symmetric pattern without duplicate entries is
// required (`err` says why not). On SIGMA_TOO_LARGE `pl` holds the split (pieces, Σ) but no numeric layout.
inline int make_plan(int n, const int64_t *colptr, const int64_t *rowval, int P, int sigma_max, Plan &pl, std::string &err) {
  char buf[256];
  pl = Plan{};
  pl.n = n; pl.P = P;
  if (n < 0 || P < 1 || P > P_MAX) { err = "bad n or piece size"; return BAD_PATTERN; }
  const int64_t nnz = n ? colptr[n] : 0;
  pl.nnz = nnz;
  // graph of the off-diagonal pattern, checked for symmetry and duplicates
  std::vector<int> aptr(n + 1, 0), adj;
  {
    std::vector<std::pair<int, int>> s;   // (column, row)
    s.reserve((size_t)nnz);
    for (int c = 0; c < n; ++c) {
      if (colptr[c + 1] < colptr[c]) { err = "colptr is not monotone"; return BAD_PATTERN; }
      for (int64_t k = colptr[c]; k < colptr[c + 1]; ++k) {
        const int64_t r = rowval[k];
        if (r < 0 || r >= n) { err = "row index out of range"; return BAD_PATTERN; }
        s.push_back({c, (int)r});
      }
    }
    std::sort(s.begin(), s.end());
    for (size_t k = 1; k < s.size(); ++k)
      if (s[k] == s[k - 1]) {
        snprintf(buf, sizeof buf, "duplicate entry (%d, %d)", s[k].second, s[k].first);
        err = buf; return BAD_PATTERN;
      }
    for (auto &p : s)
      if (p.first != p.second && !std::binary_search(s.begin(), s.end(), std::make_pair(p.second, p.first))) {
        snprintf(buf, sizeof buf, "pattern is not symmetric: (%d, %d) is stored, (%d, %d) is not", p.second, p.first, p.first, p.second);
        err = buf; return BAD_PATTERN;
      }
    for (auto &p : s) if (p.first != p.second) aptr[p.first + 1]++;
    for (int i = 0; i < n; ++i) aptr[i + 1] += aptr[i];
    adj.resize(aptr[n]);
    std::vector<int> nx(aptr.begin(), aptr.end() - 1);
    for (auto &p : s) if (p.first != p.second) adj[nx[p.first]++] = p.second;   // ascending within a node (s is sorted)
  }
  // 1. breadth-first pieces
  std::vector<int> piece(n, -1);
  int np = 0;
  std::vector<int> q;
  for (int s0 = 0; s0 < n; ++s0) {
    if (piece[s0] >= 0) continue;
    q.assign(1, s0);
    piece[s0] = np;
    int taken = 1;
    for (size_t h = 0; h < q.size() && taken < P; ++h)
      for (int k = aptr[q[h]]; k < aptr[q[h] + 1] && taken < P; ++k) {
        const int v = adj[k];
        if (piece[v] >= 0) continue;
        piece[v] = np; q.push_back(v); ++taken;
      }
    ++np;
  }
  // 2. greedy vertex cover of the cross edges
  std::vector<int> cross(n, 0);
  for (int v = 0; v < n; ++v)
    for (int k = aptr[v]; k < aptr[v + 1]; ++k) cross[v] += piece[adj[k]] != piece[v];
  std::set<std::pair<int, int>> heap;   // (-cross, node)
  for (int v = 0; v < n; ++v) if (cross[v]) heap.insert({-cross[v], v});
  std::vector<char> in_sigma(n, 0);
  while (!heap.empty()) {
    const int v = heap.begin()->second;
    heap.erase(heap.begin());
    in_sigma[v] = 1;
    for (int k = aptr[v]; k < aptr[v + 1]; ++k) {
      const int w = adj[k];
      if (in_sigma[w] || piece[w] == piece[v]) continue;   // covered before, or not a cross edge
      heap.erase({-cross[w], w});
      if (--cross[w]) heap.insert({-cross[w], w});
    }
    cross[v] = 0;
  }
  for (int v = 0; v < n; ++v) if (in_sigma[v]) pl.sigma.push_back(v);
  const int ns = (int)pl.sigma.size();
  // renumber the non-empty pieces in order of their first node
  std::vector<int> renum(np, -1);
  int npk = 0;
  pl.piece_of.assign(n, -1);
  pl.local.assign(n, -1);
  for (int v = 0; v < n; ++v) {
    if (in_sigma[v]) continue;
    if (renum[piece[v]] < 0) renum[piece[v]] = npk++;
    pl.piece_of[v] = renum[piece[v]];
  }
  pl.piece_ptr.assign(npk + 1, 0);
  for (int v = 0; v < n; ++v) if (pl.piece_of[v] >= 0) pl.piece_ptr[pl.piece_of[v] + 1]++;
  for (int i = 0; i < npk; ++i) pl.piece_ptr[i + 1] += pl.piece_ptr[i];
  pl.piece_node.resize(pl.piece_ptr[npk]);
  {
    std::vector<int> nx(pl.piece_ptr.begin(), pl.piece_ptr.end() - 1);
    for (int v = 0; v < n; ++v)
      if (pl.piece_of[v] >= 0) { const int i = pl.piece_of[v]; pl.local[v] = nx[i] - pl.piece_ptr[i]; pl.piece_node[nx[i]++] = v; }
  }
  for (int a = 0; a < ns; ++a) pl.local[pl.sigma[a]] = a;
  if (ns > sigma_max) {
    snprintf(buf, sizeof buf, "the separator has %d nodes, above the limit of %d (s^-1 is dense: the graph is not interface-like)", ns, sigma_max);
    err = buf; return SIGMA_TOO_LARGE;
  }
  // Σ_i
  pl.sig_ptr.assign(npk + 1, 0);
  for (int i = 0; i < npk; ++i) {
    std::vector<int> si;
    for (int p = pl.piece_ptr[i]; p < pl.piece_ptr[i + 1]; ++p) {
      const int v = pl.piece_node[p];
      for (int k = aptr[v]; k < aptr[v + 1]; ++k) if (in_sigma[adj[k]]) si.push_back(pl.local[adj[k]]);
    }
    std::sort(si.begin(), si.end());
    si.erase(std::unique(si.begin(), si.end()), si.end());
    pl.sig_idx.insert(pl.sig_idx.end(), si.begin(), si.end());
    pl.sig_ptr[i + 1] = (int)pl.sig_idx.size();
  }
  // slots of every Σ node (ascending slot = ascending piece), orphans
  const int nslot = pl.sig_ptr[npk];
  pl.slot_piece.resize(nslot);
  pl.slot_ptr.assign(ns + 1, 0);
  for (int i = 0; i < npk; ++i)
    for (int qq = pl.sig_ptr[i]; qq < pl.sig_ptr[i + 1]; ++qq) { pl.slot_piece[qq] = i; pl.slot_ptr[pl.sig_idx[qq] + 1]++; }
  for (int a = 0; a < ns; ++a) pl.slot_ptr[a + 1] += pl.slot_ptr[a];
  pl.slot.resize(nslot);
  {
    std::vector<int> nx(pl.slot_ptr.begin(), pl.slot_ptr.end() - 1);
    for (int qq = 0; qq < nslot; ++qq) pl.slot[nx[pl.sig_idx[qq]]++] = qq;
  }
  for (int a = 0; a < ns; ++a) if (pl.slot_ptr[a] == pl.slot_ptr[a + 1]) pl.orphan.push_back(a);
  // dense layout and the destination of every stored entry
  pl.d_off.assign(npk + 1, 0); pl.b_off.assign(npk + 1, 0); pl.s_off.assign(npk + 1, 0);
  for (int i = 0; i < npk; ++i) {
    const int64_t ni = pl.piece_ptr[i + 1] - pl.piece_ptr[i], si = pl.sig_ptr[i + 1] - pl.sig_ptr[i];
    pl.d_off[i + 1] = pl.d_off[i] + ni * ni;
    pl.b_off[i + 1] = pl.b_off[i] + ni * si;
    pl.s_off[i + 1] = pl.s_off[i] + si * si;
  }
  pl.d_total = pl.d_off[npk]; pl.b_total = pl.b_off[npk]; pl.patch_total = pl.s_off[npk];
  pl.dst.assign((size_t)nnz, -1);
  for (int c = 0; c < n; ++c)
    for (int64_t k = colptr[c]; k < colptr[c + 1]; ++k) {
      const int r = (int)rowval[k];
      const int pr = pl.piece_of[r], pc = pl.piece_of[c];
      if (pr >= 0 && pc >= 0) {                      // same piece (a cross edge has an endpoint in Σ by construction)
        const int64_t ni = pl.piece_ptr[pr + 1] - pl.piece_ptr[pr];
        pl.dst[k] = pl.d_off[pr] + pl.local[r] + (int64_t)pl.local[c] * ni;
      } else if (pr >= 0) {                          // B' entry (piece row, Σ column)
        const int64_t ni = pl.piece_ptr[pr + 1] - pl.piece_ptr[pr];
        const int *b = pl.sig_idx.data() + pl.sig_ptr[pr], *e = pl.sig_idx.data() + pl.sig_ptr[pr + 1];
        const int64_t kk = std::lower_bound(b, e, pl.local[c]) - b;
        pl.dst[k] = pl.d_total + pl.b_off[pr] + pl.local[r] + kk * ni;
      } else if (pc < 0) {                           // A_ΣΣ
        pl.dst[k] = pl.d_total + pl.b_total + pl.local[r] + (int64_t)pl.local[c] * ns;
      }
    }
  return OK;
}

}  // namespace spd
}  // namespace mi
