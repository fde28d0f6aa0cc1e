// Symbolic phase of the smoothed-aggregation hierarchy for FROZEN aggregates (amg_setup.hpp runs the numbers on it): host
// only, no HIP, so that a CPU test compiles it (tests/cpp/amg_plan_check.cpp).
//
// fem.amg_aggregate sees the values of a matrix only through `data != 0`, so on one mesh every realization has the
// aggregates, and with them every sparsity pattern of the hierarchy, of the first one. What is left per realization is
// arithmetic on fixed patterns. From the stored pattern of A_0 (sorted CSR, stored zeros are entries) and one aggregate
// array per smoothed level, agg_l[i] in 0 .. n_{l+1} - 1, this plan holds per level l < nlevels - 1:
//   tw[J] = 1 / sqrt(|agg J|)              the tentative prolongator T[i, agg(i)] = tw[agg(i)]
//   P_l     pattern(T_l) ∪ pattern(A_l T_l), sorted CSR. Every stored A_l(i, j) feeds exactly one entry, (i, agg(j)):
//           seg_ptr (nnz(P_l) + 1) / seg_src, a permutation of the entries of A_l, ascending inside a segment, so
//           P[k] = T[k] - (ω/d)_i Σ_{s in segment k} A[seg_src[s]] tw[col(k)]   summed in ascending column of A_l
//   R_l     = P_l' in sorted CSR, r_from[k]: the entry of P_l that R_l's entry k copies
//   A_l P_l and A_{l+1} = R_l (A_l P_l): the STRUCTURAL patterns (no entry is dropped because its value cancels), sorted
//   sym     of the next level: A_{l+1} entry k = (I, J) -> the entry (J, I); the pattern is structurally symmetric
//   diag    of every level: the entry (i, i) of row i, or -1
// Refusals (BAD_ARG, `err` names the numbers): a pattern of A_0 that is not sorted without duplicates or not structurally
// symmetric, an aggregate id out of range, an empty aggregate, level sizes that do not chain, a coarsest level above
// MAX_COARSE rows, a context that is one rank of several.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

namespace mi {
namespace amgp {

constexpr int MAX_COARSE = 4096;   // rows of the dense coarsest inverse (amg.hpp AMG_MAX_COARSE)
constexpr int MAX_LEVELS = 64;

struct Level {
  int n = 0, nc = 0;                       // rows of this level and of the next (nc = 0 on the coarsest level)
  std::vector<int> a_ptr, a_col, diag;     // pattern of A_l; position of (i, i) or -1
  std::vector<int> sym;                    // entry k = (i, j) -> entry (j, i)
  // below: smoothed levels only
  std::vector<int> agg;
  std::vector<double> tw;
  std::vector<int> p_ptr, p_col, seg_ptr, seg_src;
  std::vector<int> r_ptr, r_col, r_from;
  std::vector<int> ap_ptr, ap_col;
  int64_t a_nnz() const { return (int64_t)a_col.size(); }
  int64_t p_nnz() const { return (int64_t)p_col.size(); }
  int64_t ap_nnz() const { return (int64_t)ap_col.size(); }
};

struct Plan {
  int nlev = 0;
  std::vector<Level> lv;
  // 4 bytes per index and 8 per weight of everything above: what the device keeps of the plan
  int64_t bytes() const {
    int64_t b = 0;
    for (const Level &L : lv)
      b += 4 * (int64_t)(L.a_ptr.size() + L.a_col.size() + L.diag.size() + L.sym.size() + L.agg.size() + L.p_ptr.size() + L.p_col.size() +
                         L.seg_ptr.size() + L.seg_src.size() + L.r_ptr.size() + L.r_col.size() + L.r_from.size() + L.ap_ptr.size() +
                         L.ap_col.size()) +
           8 * (int64_t)L.tw.size();
    return b;
  }
};

enum Status { OK = 0, BAD_ARG = 1 };

namespace detail {
// C = A B on patterns: row i of C is the sorted union of the rows B[j], j in row i of A
inline bool structural_product(int n, const std::vector<int> &aptr, const std::vector<int> &acol, const std::vector<int> &bptr,
                               const std::vector<int> &bcol, int ncol, std::vector<int> &cptr, std::vector<int> &ccol) {
  std::vector<int> mark((size_t)ncol, -1), row;
  cptr.assign((size_t)n + 1, 0);
  ccol.clear();
  for (int i = 0; i < n; ++i) {
    row.clear();
    for (int k = aptr[i]; k < aptr[i + 1]; ++k) {
      const int j = acol[k];
      for (int q = bptr[j]; q < bptr[j + 1]; ++q) {
        const int c = bcol[q];
        if (mark[c] != i) { mark[c] = i; row.push_back(c); }
      }
    }
    std::sort(row.begin(), row.end());
    if (ccol.size() + row.size() >= (size_t)INT32_MAX) return false;
    ccol.insert(ccol.end(), row.begin(), row.end());
    cptr[(size_t)i + 1] = (int)ccol.size();
  }
  return true;
}
// sym[k] for a sorted pattern; returns the first entry without a mirror, or -1
inline int64_t mirror(int n, const std::vector<int> &ptr, const std::vector<int> &col, std::vector<int> &sym) {
  sym.assign(col.size(), -1);
  for (int i = 0; i < n; ++i)
    for (int k = ptr[i]; k < ptr[i + 1]; ++k) {
      const int j = col[k];
      const int *b = col.data() + ptr[j], *e = col.data() + ptr[j + 1];
      const int *f = std::lower_bound(b, e, i);
      if (f == e || *f != i) return k;
      sym[k] = (int)(f - col.data());
    }
  return -1;
}
inline void diagonal(int n, const std::vector<int> &ptr, const std::vector<int> &col, std::vector<int> &diag) {
  diag.assign((size_t)n, -1);
  for (int i = 0; i < n; ++i) {
    const int *b = col.data() + ptr[i], *e = col.data() + ptr[i + 1];
    const int *f = std::lower_bound(b, e, i);
    if (f != e && *f == i) diag[i] = (int)(f - col.data());
  }
}
}  // namespace detail

// rowptr (n + 1) / colidx of A_0 and agg[l] (n_l[l] entries, l < nlevels - 1), all `base`-based. rank / n_ranks: the
// context's (the hierarchy is replicated only).
inline int make_plan(int64_t n, const int64_t *rowptr, const int64_t *colidx, int64_t nlevels, const int64_t *n_l, const int64_t *const *agg,
                     int base, int rank, int n_ranks, Plan &pl, std::string &err) {
  char buf[320];
#define MI_AMGP_FAIL(...) do { std::snprintf(buf, sizeof buf, __VA_ARGS__); err = buf; pl = Plan{}; return BAD_ARG; } while (0)
  pl = Plan{};
  const char *me = "mi_amg_plan_create";
  if (n_ranks > 1) MI_AMGP_FAIL("%s: the operator is replicated only; this context is rank %d of %d", me, rank, n_ranks);
  if (base != 0 && base != 1) MI_AMGP_FAIL("%s: index_base = %d (0 or 1)", me, base);
  if (nlevels < 1 || nlevels > MAX_LEVELS) MI_AMGP_FAIL("%s: nlevels = %lld (1 <= nlevels <= %d)", me, (long long)nlevels, MAX_LEVELS);
  if (!rowptr || !colidx || !n_l || (nlevels > 1 && !agg)) MI_AMGP_FAIL("%s: NULL rowptr, colidx, n_l or array of aggregate arrays", me);
  if (n_l[0] != n) MI_AMGP_FAIL("%s: the level sizes do not chain: n_l[0] = %lld for a matrix of %lld rows", me, (long long)n_l[0], (long long)n);
  for (int64_t l = 0; l < nlevels; ++l) {
    if (n_l[l] < 1 || n_l[l] >= INT32_MAX) MI_AMGP_FAIL("%s: level %lld has n = %lld rows", me, (long long)l, (long long)n_l[l]);
    if (l && n_l[l] >= n_l[l - 1])
      MI_AMGP_FAIL("%s: the level sizes do not chain: level %lld has %lld rows after %lld", me, (long long)l, (long long)n_l[l], (long long)n_l[l - 1]);
  }
  if (n_l[nlevels - 1] > MAX_COARSE)
    MI_AMGP_FAIL("%s: the coarsest level has %lld rows, the dense inverse holds at most %d", me, (long long)n_l[nlevels - 1], MAX_COARSE);
  pl.nlev = (int)nlevels;
  pl.lv.resize((size_t)nlevels);
  {   // A_0: sorted rows without duplicates, structurally symmetric
    Level &L = pl.lv[0];
    L.n = (int)n;
    const int64_t nnz = rowptr[n] - base;
    if (rowptr[0] != base || nnz < 0 || nnz >= INT32_MAX) MI_AMGP_FAIL("%s: rowptr[0] = %lld, %lld stored entries (index_base = %d)", me, (long long)rowptr[0], (long long)nnz, base);
    L.a_ptr.resize((size_t)n + 1);
    L.a_col.resize((size_t)nnz);
    for (int64_t i = 0; i <= n; ++i) {
      const int64_t v = rowptr[i] - base;
      if (v < 0 || v > nnz || (i && v < L.a_ptr[(size_t)i - 1])) MI_AMGP_FAIL("%s: rowptr is not monotone at row %lld (%lld)", me, (long long)i, (long long)rowptr[i]);
      L.a_ptr[(size_t)i] = (int)v;
    }
    for (int64_t i = 0; i < n; ++i)
      for (int k = L.a_ptr[(size_t)i]; k < L.a_ptr[(size_t)i + 1]; ++k) {
        const int64_t c = colidx[k] - base;
        if (c < 0 || c >= n) MI_AMGP_FAIL("%s: row %lld holds column %lld, outside the %lld columns", me, (long long)i, (long long)colidx[k], (long long)n);
        if (k > L.a_ptr[(size_t)i] && c <= L.a_col[(size_t)k - 1])
          MI_AMGP_FAIL("%s: row %lld holds column %lld after column %lld: the pattern is not sorted, or has duplicates", me, (long long)i, (long long)c,
                       (long long)L.a_col[(size_t)k - 1]);
        L.a_col[(size_t)k] = (int)c;
      }
    const int64_t bad = detail::mirror(L.n, L.a_ptr, L.a_col, L.sym);
    if (bad >= 0) {
      const int i = (int)(std::upper_bound(L.a_ptr.begin(), L.a_ptr.end(), (int)bad) - L.a_ptr.begin()) - 1;
      MI_AMGP_FAIL("%s: the pattern is not structurally symmetric: entry (%d, %d) is stored, (%d, %d) is not", me, i, L.a_col[(size_t)bad], L.a_col[(size_t)bad], i);
    }
    detail::diagonal(L.n, L.a_ptr, L.a_col, L.diag);
  }
  for (int l = 0; l + 1 < pl.nlev; ++l) {
    Level &L = pl.lv[(size_t)l], &N = pl.lv[(size_t)l + 1];
    const int nl = L.n, nc = (int)n_l[l + 1];
    L.nc = nc; N.n = nc;
    if (!agg[l]) MI_AMGP_FAIL("%s: the aggregates of level %d are NULL", me, l);
    L.agg.resize((size_t)nl);
    std::vector<int> cnt((size_t)nc, 0);
    for (int i = 0; i < nl; ++i) {
      const int64_t a = agg[l][i] - base;
      if (a < 0 || a >= nc) MI_AMGP_FAIL("%s: level %d: node %d is in aggregate %lld, outside the %d aggregates", me, l, i, (long long)agg[l][i], nc);
      L.agg[(size_t)i] = (int)a;
      cnt[(size_t)a]++;
    }
    L.tw.resize((size_t)nc);
    for (int a = 0; a < nc; ++a) {
      if (!cnt[(size_t)a]) MI_AMGP_FAIL("%s: level %d: aggregate %d of %d is empty", me, l, a, nc);
      L.tw[(size_t)a] = 1.0 / std::sqrt((double)cnt[(size_t)a]);
    }
    // P and its segments, row by row: the entries of A's row ordered by (aggregate of the column, position)
    L.p_ptr.assign((size_t)nl + 1, 0);
    L.seg_ptr.assign(1, 0);
    L.seg_src.reserve(L.a_col.size());
    std::vector<std::pair<int, int>> row;
    for (int i = 0; i < nl; ++i) {
      row.clear();
      for (int k = L.a_ptr[(size_t)i]; k < L.a_ptr[(size_t)i + 1]; ++k) row.emplace_back(L.agg[(size_t)L.a_col[(size_t)k]], k);
      row.emplace_back(L.agg[(size_t)i], -1);          // T's own entry: present without a stored diagonal too
      std::sort(row.begin(), row.end());
      for (size_t q = 0; q < row.size(); ++q) {
        if (q == 0 || row[q].first != row[q - 1].first) {
          if (q) L.seg_ptr.push_back((int)L.seg_src.size());
          L.p_col.push_back(row[q].first);
        }
        if (row[q].second >= 0) L.seg_src.push_back(row[q].second);
      }
      L.seg_ptr.push_back((int)L.seg_src.size());
      L.p_ptr[(size_t)i + 1] = (int)L.p_col.size();
    }
    // (seg_ptr now has one entry per P entry plus the leading 0: the pushes above close every segment once)
    // R = P' with the source of every entry
    const size_t pn = L.p_col.size();
    L.r_ptr.assign((size_t)nc + 1, 0);
    for (int c : L.p_col) L.r_ptr[(size_t)c + 1]++;
    for (int a = 0; a < nc; ++a) L.r_ptr[(size_t)a + 1] += L.r_ptr[(size_t)a];
    L.r_col.resize(pn); L.r_from.resize(pn);
    {
      std::vector<int> next(L.r_ptr.begin(), L.r_ptr.end() - 1);
      for (int i = 0; i < nl; ++i)
        for (int k = L.p_ptr[(size_t)i]; k < L.p_ptr[(size_t)i + 1]; ++k) {
          const int q = next[(size_t)L.p_col[(size_t)k]]++;
          L.r_col[(size_t)q] = i; L.r_from[(size_t)q] = k;
        }
    }
    if (!detail::structural_product(nl, L.a_ptr, L.a_col, L.p_ptr, L.p_col, nc, L.ap_ptr, L.ap_col) ||
        !detail::structural_product(nc, L.r_ptr, L.r_col, L.ap_ptr, L.ap_col, nc, N.a_ptr, N.a_col))
      MI_AMGP_FAIL("%s: level %d: a product pattern has 2^31 entries or more", me, l);
    const int64_t bad = detail::mirror(nc, N.a_ptr, N.a_col, N.sym);
    if (bad >= 0) MI_AMGP_FAIL("%s: level %d: the pattern of the Galerkin product is not structurally symmetric at entry %lld", me, l + 1, (long long)bad);
    detail::diagonal(nc, N.a_ptr, N.a_col, N.diag);
  }
#undef MI_AMGP_FAIL
  return OK;
}

}  // namespace amgp
}  // namespace mi
