// The symbolic half of the level set-up (setup_gj.hpp), built once per mesh / partition: host only, no HIP, so that a CPU
// test compiles it (tests/cpp/setup_plan_check.cpp).
//
// `assemble_local_schurs` (EPDD.jl:667-695) wants S_d = A_ΓΓdd - A_IΓdd' A_IIdd^{-1} A_IΓdd for every subdomain and
// `get_schur_rhs` (:853-861) the condensed right-hand side w_d = A_IΓdd' A_IIdd^{-1} b_Id. The reference applies
// `apply_local_schur` (interior CG to reltol 1e-9) to every unit vector; here the interior is eliminated EXACTLY (documented
// deviation N2 of DESIGN.md §2: it only tightens S_d): the interior nodes are ordered by breadth-first levels L_0, L_1, ...
// grown from the nodes adjacent to Γ_d (the rows of A_IΓdd that hold an entry; every level sorted). A_II is block
// tridiagonal in that order, so
//     T_m = A_mm,   T_k = A_kk - C_k' T_{k+1}^{-1} C_k,   g_k = b_k - C_k' T_{k+1}^{-1} g_{k+1},      C_k = A_{k+1,k}
//     S_d = A_ΓΓ - B' T_0^{-1} B,   w_d = B' T_0^{-1} g_0,                                            B = A_IΓ[L_0, :]
// is a chain over dense blocks a few hundred wide. The plan says where every stored entry of the CSC blocks lands:
//   entry lists   (src, dst) pairs for the dense A_kk of every level and for A_ΓΓ: dense[dst] += values[src], dst
//                 column-major in the block, src an index into the value family (ii or gg) concatenated over the subdomains;
//   perm          position in level order -> index into the concatenated interior vectors, one slot per interior node (an
//                 interior node that no level reaches cannot influence S_d: the tail slots of its subdomain hold 0);
//   column form   of the sparse coupling blocks C_k (columns = nodes of level k) and B (columns = Γ_d): c_ptr / c_row / c_src,
//                 rows as positions inside their level, the entries of a column in ascending row.
// A realization (Example07:162-199) is then a run with the block values where mi_assembly_run left them.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

namespace mi {
namespace setup {

struct Input {                               // everything borrowed; indices in the caller's `base` (0 or 1)
  int64_t ndom = 0;
  int base = 0;
  const int64_t *n_gamma_d = nullptr, *n_i = nullptr;          // (ndom)
  // per subdomain the CSC patterns of A_II (n_i x n_i), A_IΓ (n_i x n_Γd) and A_ΓΓ (n_Γd x n_Γd)
  const int64_t *const *ii_ptr = nullptr, *const *ii_idx = nullptr, *const *ig_ptr = nullptr, *const *ig_idx = nullptr;
  const int64_t *const *gg_ptr = nullptr, *const *gg_idx = nullptr;
};

struct Dom {
  int n_g = 0, n_i = 0, nlev = 0;
  std::vector<int> lev_off;              // [nlev + 1] offsets of the levels in the permuted interior
  std::vector<long long> d_e0;           // [nlev + 1]: level k's A_kk is the range [d_e0[k], d_e0[k + 1]) of the entry lists
  long long g_e0 = 0, g_e1 = 0;          // ... and A_ΓΓ the range [g_e0, g_e1)
  long long ii_val_off = 0, ig_val_off = 0, gg_val_off = 0, bi_off = 0, s_off = 0, w_off = 0;
  int max_lev = 0;
  // column form of the coupling blocks: for level k the columns of C_k = A_{k+1,k}, as offsets into the plan-wide arrays
  // c_ptr / c_row / c_src; [nlev - 1] entries; then B = A_IΓ[L_0, :] by Γ_d column
  std::vector<int> cptr_off;
  int bptr_off = 0;
};

struct Plan {
  int ndom = 0;
  std::vector<Dom> dom;
  std::vector<int> src_h, dst_h, perm_h;           // entry lists of A_kk and A_ΓΓ of all subdomains; interior permutation (concatenated)
  std::vector<int> c_ptr_h, c_row_h, c_src_h;      // column form of all C_k and B
  long long n_ii = 0, n_ig = 0, n_gg = 0, n_bi = 0, n_s = 0, n_w = 0;   // Σ stored entries of the three families, Σ n_i, Σ n_Γd², Σ n_Γd
};

enum Status { OK = 0, BAD_ARG = 1 };

#define MI_SETUP_FAIL(...) do { char buf_[320]; std::snprintf(buf_, sizeof buf_, __VA_ARGS__); err = buf_; return BAD_ARG; } while (0)
// `dst = (int)v` for lo <= v < hi, a refusal otherwise
#define MI_SETUP_I32(dst, v, lo, hi, what)                                                                                          \
  do {                                                                                                                              \
    const int64_t v_ = (v);                                                                                                         \
    if (v_ < (lo) || v_ >= (hi)) MI_SETUP_FAIL("%s: index %lld outside [%lld, %lld)", what, (long long)v_, (long long)(lo), (long long)(hi)); \
    dst = (int)v_;                                                                                                                  \
  } while (0)

inline int make_plan(const Input &in, Plan &P, std::string &err) {
  P = Plan{};
  P.ndom = (int)in.ndom;
  const int base = in.base;
  for (int64_t d = 0; d < in.ndom; ++d) {
    Dom D;
    D.n_g = (int)in.n_gamma_d[d]; D.n_i = (int)in.n_i[d];
    const int ng = D.n_g, ni = D.n_i;
    if (ng < 0 || ni < 0) MI_SETUP_FAIL("setup plan: negative size");
    const int64_t *ip = in.ii_ptr[d], *ix = in.ii_idx[d], *gp = in.ig_ptr[d], *gx = in.ig_idx[d], *sp = in.gg_ptr[d], *sx = in.gg_idx[d];
    if ((ni && (!ip || !ix)) || !gp || !sp) MI_SETUP_FAIL("setup plan: NULL block arrays for subdomain %lld", (long long)d);
    const int64_t nnz_ii = ni ? ip[ni] - base : 0, nnz_ig = gp[ng] - base, nnz_gg = sp[ng] - base;
    if (nnz_ii < 0 || nnz_ig < 0 || nnz_gg < 0 || nnz_ii >= INT32_MAX) MI_SETUP_FAIL("setup plan: bad colptr");
    D.ii_val_off = P.n_ii; D.ig_val_off = P.n_ig; D.gg_val_off = P.n_gg; D.bi_off = P.n_bi; D.s_off = P.n_s; D.w_off = P.n_w;
    if (P.n_ii + nnz_ii >= INT32_MAX || P.n_ig + nnz_ig >= INT32_MAX) MI_SETUP_FAIL("setup plan: more than 2^31 stored entries");
    // breadth-first levels from the interior nodes adjacent to Γ_d (rows of A_IΓdd that hold an entry)
    std::vector<int> level(ni, -1), order, frontier;
    order.reserve(ni);
    for (int64_t k = 0; k < nnz_ig; ++k) {
      int r;
      MI_SETUP_I32(r, gx[k] - base, 0, ni, "A_IΓ rowval");
      if (level[r] < 0) { level[r] = 0; frontier.push_back(r); }
    }
    std::sort(frontier.begin(), frontier.end());
    D.lev_off.push_back(0);
    while (!frontier.empty()) {
      for (int v : frontier) order.push_back(v);
      D.lev_off.push_back((int)order.size());
      std::vector<int> next;
      const int lv = (int)D.lev_off.size() - 1;
      for (int v : frontier)
        for (int64_t k = ip[v] - base; k < ip[v + 1] - base; ++k) {
          int u;
          MI_SETUP_I32(u, ix[k] - base, 0, ni, "A_II rowval");
          if (level[u] < 0) { level[u] = lv; next.push_back(u); }
        }
      std::sort(next.begin(), next.end());
      frontier.swap(next);
    }
    D.nlev = (int)D.lev_off.size() - 1;
    auto width = [&](int l) { return D.lev_off[l + 1] - D.lev_off[l]; };
    std::vector<int> pos(ni, -1);   // position inside its level
    for (int l = 0; l < D.nlev; ++l) {
      for (int q = D.lev_off[l]; q < D.lev_off[l + 1]; ++q) pos[order[q]] = q - D.lev_off[l];
      D.max_lev = std::max(D.max_lev, width(l));
    }
    // A_II, column by column: an entry inside a level goes to that level's entry list (index into the value family, position
    // in the dense block, column-major); one from level k to level k + 1 to column pos[col] of C_k as (row, value index)
    std::vector<std::vector<std::pair<int, int>>> Dl(D.nlev);
    std::vector<std::vector<std::vector<std::pair<int, int>>>> Cl(std::max(0, D.nlev - 1));
    for (int l = 0; l + 1 < D.nlev; ++l) Cl[l].resize(width(l));
    for (int col = 0; col < ni; ++col) {
      const int lc = level[col];
      if (lc < 0) continue;   // not connected to Γ_d: cannot influence S_d
      for (int64_t k = ip[col] - base; k < ip[col + 1] - base; ++k) {
        const int row = (int)(ix[k] - base), lr = level[row];
        const int srcv = (int)(P.n_ii + k);
        if (lr == lc) Dl[lc].push_back({srcv, pos[row] + pos[col] * width(lc)});
        else if (lr == lc + 1) Cl[lc][pos[col]].push_back({pos[row], srcv});
        // lr == lc - 1: the transposed twin, not stored (symmetric); |lr - lc| > 1 cannot occur
        else if (lr >= 0 && lr != lc - 1) MI_SETUP_FAIL("setup plan: A_II is not block tridiagonal over the BFS levels (not symmetric?)");
      }
    }
    for (int l = 0; l + 1 < D.nlev; ++l) {
      D.cptr_off.push_back((int)P.c_ptr_h.size());
      for (auto &c : Cl[l]) {
        P.c_ptr_h.push_back((int)P.c_row_h.size());
        std::sort(c.begin(), c.end());
        for (auto &e : c) { P.c_row_h.push_back(e.first); P.c_src_h.push_back(e.second); }
      }
      P.c_ptr_h.push_back((int)P.c_row_h.size());
    }
    for (int l = 0; l < D.nlev; ++l) {
      D.d_e0.push_back((long long)P.src_h.size());
      for (auto &e : Dl[l]) { P.src_h.push_back(e.first); P.dst_h.push_back(e.second); }
    }
    D.d_e0.push_back((long long)P.src_h.size());
    // B = A_IΓ[L_0, :] (n_0 x n_Γd) from the CSC arrays of A_IΓdd, in stored order
    D.bptr_off = (int)P.c_ptr_h.size();
    for (int col = 0; col < ng; ++col) {
      P.c_ptr_h.push_back((int)P.c_row_h.size());
      for (int64_t k = gp[col] - base; k < gp[col + 1] - base; ++k) {
        P.c_row_h.push_back(pos[(int)(gx[k] - base)]); P.c_src_h.push_back((int)(P.n_ig + k));
      }
    }
    P.c_ptr_h.push_back((int)P.c_row_h.size());
    D.g_e0 = (long long)P.src_h.size();
    for (int col = 0; col < ng; ++col)
      for (int64_t k = sp[col] - base; k < sp[col + 1] - base; ++k) {
        int row;
        MI_SETUP_I32(row, sx[k] - base, 0, ng, "A_ΓΓ rowval");
        P.src_h.push_back((int)(P.n_gg + k)); P.dst_h.push_back(row + col * std::max(ng, 1));
      }
    D.g_e1 = (long long)P.src_h.size();
    for (int v : order) P.perm_h.push_back((int)(P.n_bi + v));
    for (int q = (int)order.size(); q < ni; ++q) P.perm_h.push_back(0);   // keep one slot per interior node (unreached: unused)
    P.n_ii += nnz_ii; P.n_ig += nnz_ig; P.n_gg += nnz_gg; P.n_bi += ni; P.n_s += (long long)ng * ng; P.n_w += ng;
    P.dom.push_back(std::move(D));
  }
  if (P.src_h.size() >= (size_t)INT32_MAX) MI_SETUP_FAIL("setup plan: too many entries");
  return OK;
}

#undef MI_SETUP_I32
#undef MI_SETUP_FAIL

// The row form of an nr x nc block from its column form (ptr: nc + 1 offsets into row / src), APPENDED to r_ptr / r_col /
// r_src: nr + 1 offsets into r_col / r_src, the entries of a row in ascending column. (The back-substitutions multiply by
// C_k and B, the elimination by their transposes.)
inline void row_form(int nr, int nc, const int *ptr, const int *row, const int *src, std::vector<int> &r_ptr, std::vector<int> &r_col,
                     std::vector<int> &r_src) {
  const size_t p0 = r_ptr.size(), e0 = r_col.size();
  r_ptr.resize(p0 + (size_t)nr + 1, 0);
  int *rp = r_ptr.data() + p0;
  for (int p = ptr[0]; p < ptr[nc]; ++p) ++rp[row[p] + 1];
  rp[0] = (int)e0;
  for (int i = 0; i < nr; ++i) rp[i + 1] += rp[i];
  r_col.resize(e0 + (size_t)(ptr[nc] - ptr[0])); r_src.resize(r_col.size());
  std::vector<int> fill(rp, rp + nr);
  for (int j = 0; j < nc; ++j)
    for (int p = ptr[j]; p < ptr[j + 1]; ++p) {
      const int at = fill[row[p]]++;
      r_col[at] = j; r_src[at] = src[p];
    }
}

}  // namespace setup
}  // namespace mi
