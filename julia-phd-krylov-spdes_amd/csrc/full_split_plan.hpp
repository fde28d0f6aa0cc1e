// The interior/Γ split of a full system that the LORASC (lorasc.hpp) and the Neumann-Neumann induced (nn_induced.hpp)
// preconditioner share: host only, no HIP, so that a CPU test compiles it (tests/cpp/full_split_check.cpp).
//
// x is indexed like the rows of A; pos_I (the interiors concatenated, subdomain after subdomain) and pos_Γ say where the
// unknowns sit in it and are together a permutation of the rows. The stacked coupling blocks A_IΓ (one CSC matrix per
// subdomain, n_i[d] rows; values in the caller's concatenated order, entry k of subdomain d at voff[d] + k) get two forms
// that point into those values:
//   column form  per Γ node g the SEGMENTS gseg_ptr[g] .. gseg_ptr[g + 1]: the subdomains that hold a column for g, in
//                ascending d, empty columns skipped; a segment's entries seg_ptr[s] .. seg_ptr[s + 1] in stored order:
//                c_row = row in the concatenated interior vector, c_src = index into the values   (A_IΓ' y, per Γ node)
//   row form     per interior row (it belongs to one subdomain) its entries r_ptr[i] .. r_ptr[i + 1] in ascending stored
//                column j of that subdomain: r_loc = goff[d] + j, r_gam = the Γ node of the column, r_src   (A_IΓ x, per row)
// Which Γ node a column stands for is the one thing that differs:
//   identity form  gather == NULL: every subdomain has n_gamma columns, column j is Γ node j (LORASC's A_IΓd); goff = 0,
//                  so r_loc = r_gam. The holders of a node are found by walking d: no table of n_gamma x ndom entries.
//   gathered form  subdomain d has n_gamma_d[d] columns, column j is Γ node gather[d][j] (the induced operator's A_IΓdd);
//                  goff[d] = Σ_{e < d} n_gamma_e, node_cnt[g] must be the number of subdomains that hold g.
// The gathered plan of (A_IΓdd, gather) and the identity plan of the same blocks scattered to Γ-global columns agree in the
// column form and in r_ptr / r_gam wherever every gather list ascends, and in the row form's set of entries always.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace mi {
namespace split {

struct Input {                               // everything borrowed; indices in the caller's `base` (0 or 1)
  int64_t ndom = 0, n = 0, n_gamma = 0;
  int base = 0;
  const int64_t *n_i = nullptr;              // (ndom)
  const int64_t *const *pos_I = nullptr;     // pos_I[d] (n_i[d]); may be NULL where n_i[d] == 0
  const int64_t *pos_g = nullptr;            // (n_gamma)
  const int64_t *const *colptr = nullptr, *const *rowval = nullptr;   // per subdomain
  const double *const *nzval = nullptr;      // only looked at for NULL
  const int64_t *n_gamma_d = nullptr;        // gathered form: (ndom)
  const int64_t *const *gather = nullptr;    // gathered form: gather[d] (n_gamma_d[d]); NULL: identity form
  const int64_t *node_cnt = nullptr;         // gathered form: (n_gamma)
  const int64_t *plan_n_i = nullptr;         // (ndom) what the set-up plan holds; NULL: not checked
  const int64_t *plan_n_gamma_d = nullptr;   // (ndom) gathered form only; NULL: not checked
};

struct Plan {
  int n_I = 0, n_g = 0;
  int64_t nnz = 0, totg = 0;                 // totg: length of the vector r_loc points into (Σ n_gamma_d, or n_gamma)
  std::vector<int> pos_I, pos_g, gseg_ptr, seg_ptr, c_row, c_src, r_ptr, r_loc, r_gam, r_src;
  std::vector<int64_t> voff, ioff, goff;     // (ndom + 1) offsets of a subdomain's values, interior rows, local columns
};

enum Status { OK = 0, BAD_ARG = 1 };

#define MI_SPLIT_FAIL(...) do { char buf_[320]; std::snprintf(buf_, sizeof buf_, __VA_ARGS__); err = buf_; return BAD_ARG; } while (0)

// the sizes and top-level pointers; `others_ok`: the caller's own pointers, reported in the same words
inline int check_input(const Input &in, bool others_ok, std::string &err) {
  const bool gathered_ok = !in.gather || (in.n_gamma_d && in.node_cnt);
  if (!others_ok || !gathered_ok || in.ndom <= 0 || in.n <= 0 || in.n >= INT32_MAX || in.n_gamma <= 0 || !in.n_i || !in.pos_I || !in.pos_g ||
      !in.colptr || !in.rowval || !in.nzval || (in.base != 0 && in.base != 1))
    MI_SPLIT_FAIL("NULL argument, bad size or index_base (ndom = %lld, n = %lld, n_gamma = %lld, index_base = %d)", (long long)in.ndom,
                  (long long)in.n, (long long)in.n_gamma, in.base);
  return OK;
}

inline int make_plan(const Input &in, Plan &pl, std::string &err) {
  pl = Plan{};
  if (check_input(in, true, err)) return BAD_ARG;
  const int64_t ndom = in.ndom, n = in.n, n_gamma = in.n_gamma;
  const int base = in.base;
  const bool gathered = in.gather != nullptr;
  auto ncol = [&](int64_t d) { return gathered ? in.n_gamma_d[d] : n_gamma; };
  auto node = [&](int64_t d, int64_t j) { return gathered ? in.gather[d][j] - base : j; };
  // 1. the sizes against the set-up plan; 2. n
  int64_t tot = 0, totg = 0;
  for (int64_t d = 0; d < ndom; ++d) {
    if (in.plan_n_i && in.n_i[d] != in.plan_n_i[d])
      MI_SPLIT_FAIL("n_i[%lld] = %lld, the plan's subdomain has %lld interior nodes", (long long)d, (long long)in.n_i[d], (long long)in.plan_n_i[d]);
    if (gathered && in.plan_n_gamma_d && in.n_gamma_d[d] != in.plan_n_gamma_d[d])
      MI_SPLIT_FAIL("n_gamma_d[%lld] = %lld, the plan's subdomain has %lld interface nodes", (long long)d, (long long)in.n_gamma_d[d],
                    (long long)in.plan_n_gamma_d[d]);
    if (in.n_i[d] < 0 || ncol(d) < 0) MI_SPLIT_FAIL("n_i[%lld] = %lld or n_gamma_d[%lld] = %lld is negative", (long long)d, (long long)in.n_i[d], (long long)d, (long long)ncol(d));
    tot += in.n_i[d];
    if (gathered) totg += in.n_gamma_d[d];
  }
  if (tot <= 0 || tot + n_gamma != n) MI_SPLIT_FAIL("n = %lld is not Σ n_i + n_gamma = %lld (the interiors and Γ together are every row)", (long long)n, (long long)(tot + n_gamma));
  if (totg >= INT32_MAX) MI_SPLIT_FAIL("Σ n_gamma_d = %lld is too large", (long long)totg);
  const int n_I = (int)tot, n_g = (int)n_gamma;
  pl.n_I = n_I; pl.n_g = n_g; pl.totg = gathered ? totg : n_gamma;
  // 3. the two maps: together a permutation of 0 .. n-1
  pl.pos_I.resize((size_t)n_I); pl.pos_g.resize((size_t)n_g);
  {
    std::vector<char> seen((size_t)n, 0);
    size_t q = 0;
    for (int64_t d = 0; d <= ndom; ++d) {     // d == ndom: pos_Γ
      const int64_t *p = d < ndom ? in.pos_I[d] : in.pos_g, cnt = d < ndom ? in.n_i[d] : n_gamma;
      if (cnt && !p) MI_SPLIT_FAIL("pos_I[%lld] is NULL although the subdomain has %lld interior nodes", (long long)d, (long long)cnt);
      for (int64_t i = 0; i < cnt; ++i, ++q) {
        const int64_t v = p[i] - base;
        if (v < 0 || v >= n) MI_SPLIT_FAIL("%s index %lld out of range (n = %lld rows)",d < ndom ? "pos_I" : "pos_gamma", (long long)p[i], (long long)n);
        if (seen[(size_t)v]) MI_SPLIT_FAIL("pos_I and pos_gamma are not a permutation of the rows: index %lld appears twice", (long long)p[i]);
        seen[(size_t)v] = 1;
        (d < ndom ? pl.pos_I[q] : pl.pos_g[(size_t)i]) = (int)v;
      }
    }
  }
  // 4. gather lists: inside [0, n_gamma), unique per subdomain, and cnt[g] = the number of subdomains that hold g
  std::vector<int> mult;
  if (gathered) {
    mult.assign((size_t)n_g, 0);
    std::vector<int> last((size_t)n_g, -1);
    for (int64_t d = 0; d < ndom; ++d) {
      if (in.n_gamma_d[d] && !in.gather[d]) MI_SPLIT_FAIL("gather_idx[%lld] is NULL although n_gamma_d is %lld", (long long)d, (long long)in.n_gamma_d[d]);
      for (int64_t l = 0; l < in.n_gamma_d[d]; ++l) {
        const int64_t g = node(d, l);
        if (g < 0 || g >= n_gamma)
          MI_SPLIT_FAIL("gather_idx[%lld][%lld] = %lld lies outside the interface indices [%d, %lld)", (long long)d, (long long)l, (long long)(g + base), base, (long long)(n_gamma + base));
        if (last[(size_t)g] == (int)d) MI_SPLIT_FAIL("gather_idx[%lld] repeats the interface index %lld", (long long)d, (long long)(g + base));
        last[(size_t)g] = (int)d;
        ++mult[(size_t)g];
      }
    }
    for (int64_t g = 0; g < n_gamma; ++g)
      if (in.node_cnt[g] != mult[(size_t)g])
        MI_SPLIT_FAIL("node_gamma_cnt[%lld] = %lld, but %d subdomain(s) hold that interface node in their gather_idx", (long long)g,
                      (long long)in.node_cnt[g], mult[(size_t)g]);
  }
  // 5. the CSC arrays
  pl.voff.assign((size_t)ndom + 1, 0); pl.ioff.assign((size_t)ndom + 1, 0); pl.goff.assign((size_t)ndom + 1, 0);
  const std::vector<int64_t> &voff = pl.voff, &ioff = pl.ioff, &goff = pl.goff;
  for (int64_t d = 0; d < ndom; ++d) {
    const int64_t *cp = in.colptr[d];
    if (!cp) MI_SPLIT_FAIL("ig_colptr[%lld] is NULL (every subdomain needs its column pointers)", (long long)d);
    if (cp[0] != base) MI_SPLIT_FAIL("ig_colptr[%lld][0] = %lld is not index_base = %d", (long long)d, (long long)cp[0], base);
    for (int64_t j = 0; j < ncol(d); ++j)
      if (cp[j + 1] < cp[j]) MI_SPLIT_FAIL("ig_colptr[%lld] decreases at column %lld (%lld after %lld)", (long long)d, (long long)j, (long long)cp[j + 1], (long long)cp[j]);
    const int64_t nz = cp[ncol(d)] - base;
    if (nz && (!in.rowval[d] || !in.nzval[d])) MI_SPLIT_FAIL("ig_rowval / ig_nzval [%lld] is NULL with %lld stored entries", (long long)d, (long long)nz);
    pl.voff[d + 1] = voff[d] + nz; pl.ioff[d + 1] = ioff[d] + in.n_i[d]; pl.goff[d + 1] = gathered ? goff[d] + in.n_gamma_d[d] : 0;
    if (voff[d + 1] >= INT32_MAX) MI_SPLIT_FAIL("more than 2^31 stored entries (%lld up to subdomain %lld)", (long long)voff[d + 1], (long long)d);
    for (int64_t k = 0; k < nz; ++k) {
      const int64_t r = in.rowval[d][k] - base;
      if (r < 0 || r >= in.n_i[d]) MI_SPLIT_FAIL("ig_rowval[%lld] holds row %lld out of range (n_i = %lld)", (long long)d, (long long)(r + base), (long long)in.n_i[d]);
    }
  }
  const int64_t nnz = pl.nnz = voff[ndom];
  // column form
  pl.gseg_ptr.resize((size_t)n_g + 1); pl.c_row.resize((size_t)nnz); pl.c_src.resize((size_t)nnz);
  size_t e = 0;
  auto column = [&](int64_t d, int64_t j) {
    const int64_t a = in.colptr[d][j] - base, b = in.colptr[d][j + 1] - base;
    if (a == b) return;      // an empty column subtracts +0: nothing changes
    pl.seg_ptr.push_back((int)e);
    for (int64_t k = a; k < b; ++k, ++e) { pl.c_row[e] = (int)(ioff[d] + (in.rowval[d][k] - base)); pl.c_src[e] = (int)(voff[d] + k); }
  };
  if (gathered) {            // holders of every Γ node: (subdomain, local column), subdomain ascending
    std::vector<int> hp((size_t)n_g + 1, 0);
    for (int g = 0; g < n_g; ++g) hp[g + 1] = hp[g] + mult[g];
    std::vector<int> hd((size_t)totg), hl((size_t)totg), fill(hp.begin(), hp.end() - 1);
    for (int64_t d = 0; d < ndom; ++d)
      for (int64_t l = 0; l < in.n_gamma_d[d]; ++l) { const int at = fill[(size_t)node(d, l)]++; hd[at] = (int)d; hl[at] = (int)l; }
    for (int g = 0; g < n_g; ++g) {
      pl.gseg_ptr[g] = (int)pl.seg_ptr.size();
      for (int h = hp[g]; h < hp[g + 1]; ++h) column(hd[h], hl[h]);
    }
  } else {
    for (int g = 0; g < n_g; ++g) {
      pl.gseg_ptr[g] = (int)pl.seg_ptr.size();
      for (int64_t d = 0; d < ndom; ++d) column(d, g);
    }
  }
  pl.gseg_ptr[n_g] = (int)pl.seg_ptr.size();
  pl.seg_ptr.push_back((int)e);
  // row form: a subdomain's columns in ascending stored order, so each row fills in ascending column
  pl.r_ptr.assign((size_t)n_I + 1, 0); pl.r_loc.resize((size_t)nnz); pl.r_gam.resize((size_t)nnz); pl.r_src.resize((size_t)nnz);
  for (int64_t k = 0; k < nnz; ++k) ++pl.r_ptr[(size_t)pl.c_row[k] + 1];
  for (int i = 0; i < n_I; ++i) pl.r_ptr[i + 1] += pl.r_ptr[i];
  std::vector<int> fill(pl.r_ptr.begin(), pl.r_ptr.end() - 1);
  for (int64_t d = 0; d < ndom; ++d)
    for (int64_t j = 0; j < ncol(d); ++j)
      for (int64_t k = in.colptr[d][j] - base; k < in.colptr[d][j + 1] - base; ++k) {
        const int at = fill[(size_t)(ioff[d] + (in.rowval[d][k] - base))]++;
        pl.r_loc[at] = (int)(goff[d] + j); pl.r_gam[at] = (int)node(d, j); pl.r_src[at] = (int)(voff[d] + k);
      }
  return OK;
}

#undef MI_SPLIT_FAIL

}  // namespace split
}  // namespace mi
