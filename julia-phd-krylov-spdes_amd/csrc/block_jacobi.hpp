// Block-Jacobi preconditioner on the full system: the reference's `BJPreconditioner(nb, A)` (MyPreconditioners/
// BJPreconditioner.jl:1-32), the M of pcg / defpcg / eigpcg / eigdefpcg on `A` in Examples 06, 09 (`bj$(nbj)_0`), 15, 17, 19:
//     bsize = floor(n / nb);  slice(i) = (i-1) bsize + 1 : i bsize  for i < nb,  (i-1) bsize + 1 : n  for i = nb
//     y[slice(i)] = cholesky(A[slice(i), slice(i)]) \ x[slice(i)]
// Every block B_d = A[slice, slice] is solved EXACTLY by the level elimination of setup_gj.hpp used as a complete block
// LDL' of a matrix that has no interface of its own:
//   symbolic (host, once per pattern; `bj::make_split` below): a seed set G_d of the slice, the rest I_d; the set-up plan
//     with (A_II, A_IΓ, A_ΓΓ) := (B[I,I], B[I,G], B[G,G]) grows its breadth-first levels in I_d from the nodes next to G_d.
//     Default seeds, per connected component of the graph of B_d (ascending lowest node): the nodes with a stored entry of A
//     in a column < lo; else those with one in a column >= hi; else the component's lowest node. One front per component
//     keeps the levels about one grid line wide on lexicographic numberings, and every node is reached.
//   numeric (device, per set of values): one gather of A's nzval into the plan's ii / ig / gg families, the plan's run with
//     the level inverses Z_k kept (S_G = B_GG - B_GI B_II^-1 B_IG per block), S_G^-1 by the same Gauss-Jordan kernels with
//     mi_nn_pinv's probe certificate (the plain inverse only: S_G of an SPD A is SPD). A factor that is not finite, has a
//     non-positive diagonal entry in a kept inverse or fails the certificate is MI_ERR_SINGULAR, and the previous factor stays.
//   apply (3 steps + 2 launches; no atomics, fixed summation orders: two applies give the same bits):
//     forward   g_m = r_m,  g_k = r_k - C_k' (Z_{k+1} g_{k+1})          k_lv_zg / k_lv_g, reading r through perm ∘ pos
//     Γ step    y = Z_0 g_0                                              k_bj_zg0
//               t_G = r_G - B' y (LDS),  u_G = S_G^-1 t_G                k_bj_gamma
//     level 0   u_0 = Z_0 (g_0 - B u_G)                                  k_bj_back0 (k_lv_back with the row form of B)
//     backward  u_{k+1} = Z_{k+1} (g_{k+1} - C_k u_k)                    k_lv_back
//     scatter   z[row of node] = u, I and G together                    k_bj_scatter
//   Every kept Z_k is read twice per apply (Z_0 in the Γ step and at level 0), S_G^-1 once — against four reads of every
//   Z_k in the composed form (NnInducedOp, MI_NNI_ASSEMBLED, disjoint blocks, cnt = 1: two level solves).
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace mi {
namespace bj {

struct Split {
  int n = 0, nb = 0;
  std::vector<int> lo;                                  // [nb + 1] first row of every block
  std::vector<std::vector<int>> G, I;                   // block-local nodes, ascending
  std::vector<int> ncomp;                               // connected components of every block's graph
  // the blocks of the set-up plan per slice (CSC, local indices from 0) ...
  std::vector<std::vector<int64_t>> ii_ptr, ii_idx, ig_ptr, ig_idx, gg_ptr, gg_idx;
  // ... and where each of their values sits in A's nzval, concatenated over the blocks (the plan's value families)
  std::vector<int> map_ii, map_ig, map_gg;
};

// first row of block d (0-based) by the reference's slice rule
inline int64_t slice_lo(int64_t n, int64_t nb, int64_t d) { return d >= nb ? n : d * (n / nb); }

// colptr / rowval: CSC pattern of A with indices from 0. seed_ptr / seed_idx (from 0; NULL: the default rule): explicit
// seeds per block. Returns false with `err` set on a refusal.
inline bool make_split(int64_t n, const int64_t *cp, const int64_t *ri, int64_t nb, const int64_t *seed_ptr, const int64_t *seed_idx,
                       int base, Split &S, std::string &err) {
  auto fail = [&](const std::string &m) { err = m; return false; };
  auto str = [](long long v) { return std::to_string(v); };
  if (nb < 1 || nb > n) return fail("nb = " + str(nb) + " blocks for n = " + str(n) + " rows (1 <= nb <= n)");
  const int64_t nnz = cp[n];
  for (int64_t j = 0; j < n; ++j)
    if (cp[j + 1] < cp[j]) return fail("colptr decreases at column " + str(j + base));
  for (int64_t k = 0; k < nnz; ++k)
    if (ri[k] < 0 || ri[k] >= n) return fail("rowval holds row " + str(ri[k] + base) + " out of range (n = " + str(n) + ")");
  {   // structural symmetry: every column's sorted rows equal the transposed pattern's
    std::vector<int64_t> tp((size_t)n + 1, 0);
    for (int64_t k = 0; k < nnz; ++k) ++tp[(size_t)ri[k] + 1];
    for (int64_t i = 0; i < n; ++i) tp[i + 1] += tp[i];
    std::vector<int64_t> fill(tp.begin(), tp.end() - 1), tr((size_t)nnz);
    for (int64_t j = 0; j < n; ++j)
      for (int64_t k = cp[j]; k < cp[j + 1]; ++k) tr[(size_t)fill[(size_t)ri[k]]++] = j;
    std::vector<int64_t> col;
    for (int64_t j = 0; j < n; ++j) {
      col.assign(ri + cp[j], ri + cp[j + 1]);
      std::sort(col.begin(), col.end());
      if ((int64_t)col.size() != tp[j + 1] - tp[j] || !std::equal(col.begin(), col.end(), tr.begin() + tp[j]))
        return fail("the pattern is not structurally symmetric: column " + str(j + base) + " holds " + str((long long)col.size()) +
                    " entries, row " + str(j + base) + " holds " + str(tp[j + 1] - tp[j]) + " or other ones");
    }
  }
  S = Split{};
  S.n = (int)n; S.nb = (int)nb;
  S.lo.resize((size_t)nb + 1);
  for (int64_t d = 0; d <= nb; ++d) S.lo[(size_t)d] = (int)slice_lo(n, nb, d);
  S.G.resize(nb); S.I.resize(nb); S.ncomp.assign(nb, 0);
  S.ii_ptr.resize(nb); S.ii_idx.resize(nb); S.ig_ptr.resize(nb); S.ig_idx.resize(nb); S.gg_ptr.resize(nb); S.gg_idx.resize(nb);
  std::vector<int> comp, stack, gl, il;
  std::vector<char> seed;
  for (int64_t d = 0; d < nb; ++d) {
    const int lo = S.lo[d], hi = S.lo[d + 1], m = hi - lo;
    seed.assign(m, 0);
    if (seed_ptr) {
      if (seed_ptr[d + 1] < seed_ptr[d]) return fail("seed_ptr decreases at block " + str(d + base));
      for (int64_t q = seed_ptr[d]; q < seed_ptr[d + 1]; ++q) {
        const int64_t v = seed_idx[q];
        if (v < 0 || v >= m) return fail("block " + str(d + base) + ": seed " + str(v + base) + " lies outside the block's " + str(m) + " nodes");
        if (seed[(size_t)v]) return fail("block " + str(d + base) + ": seed " + str(v + base) + " appears twice");
        seed[(size_t)v] = 1;
      }
    }
    // components of the graph of B_d in ascending order of their lowest node (A's columns are B_d's adjacency lists)
    comp.assign(m, -1);
    int nc = 0;
    for (int r = 0; r < m; ++r) {
      if (comp[r] >= 0) continue;
      std::vector<int> nodes;
      comp[r] = nc; stack.assign(1, r);
      while (!stack.empty()) {
        const int v = stack.back(); stack.pop_back();
        nodes.push_back(v);
        for (int64_t k = cp[lo + v]; k < cp[lo + v + 1]; ++k) {
          const int64_t u = ri[k] - lo;
          if (u >= 0 && u < m && comp[(size_t)u] < 0) { comp[(size_t)u] = nc; stack.push_back((int)u); }
        }
      }
      ++nc;
      if (seed_ptr) {
        bool any = false;
        for (int v : nodes) any = any || seed[v];
        if (!any) return fail("block " + str(d + base) + ": the component of node " + str(r + base) + " (row " + str(lo + r + base) + ", " +
                              str((long long)nodes.size()) + " nodes) holds no seed");
        continue;
      }
      bool low = false, high = false;
      for (int v : nodes)
        for (int64_t k = cp[lo + v]; k < cp[lo + v + 1]; ++k) { low = low || ri[k] < lo; high = high || ri[k] >= hi; }
      if (!low && !high) { seed[r] = 1; continue; }
      for (int v : nodes)
        for (int64_t k = cp[lo + v]; k < cp[lo + v + 1]; ++k)
          if (low ? ri[k] < lo : ri[k] >= hi) { seed[v] = 1; break; }
    }
    S.ncomp[d] = nc;
    gl.assign(m, -1); il.assign(m, -1);
    for (int v = 0; v < m; ++v) {
      if (seed[v]) { gl[v] = (int)S.G[d].size(); S.G[d].push_back(v); }
      else { il[v] = (int)S.I[d].size(); S.I[d].push_back(v); }
    }
    auto &ip = S.ii_ptr[d], &ix = S.ii_idx[d], &gp = S.ig_ptr[d], &gx = S.ig_idx[d], &sp = S.gg_ptr[d], &sx = S.gg_idx[d];
    ip.push_back(0); gp.push_back(0); sp.push_back(0);
    for (int v : S.I[d]) {
      for (int64_t k = cp[lo + v]; k < cp[lo + v + 1]; ++k) {
        const int64_t u = ri[k] - lo;
        if (u >= 0 && u < m && il[(size_t)u] >= 0) { ix.push_back(il[(size_t)u]); S.map_ii.push_back((int)k); }
      }
      ip.push_back((int64_t)ix.size());
    }
    for (int v : S.G[d]) {
      for (int64_t k = cp[lo + v]; k < cp[lo + v + 1]; ++k) {
        const int64_t u = ri[k] - lo;
        if (u < 0 || u >= m) continue;
        if (il[(size_t)u] >= 0) { gx.push_back(il[(size_t)u]); S.map_ig.push_back((int)k); }
        else { sx.push_back(gl[(size_t)u]); S.map_gg.push_back((int)k); }
      }
      gp.push_back((int64_t)gx.size()); sp.push_back((int64_t)sx.size());
    }
  }
  return true;
}

}  // namespace bj
}  // namespace mi

#ifdef __HIPCC__
#include "setup_gj.hpp"

namespace mi {

#pragma clang fp contract(fast)
// vals[k] = nzval[map[k]]: A's values into the plan's three value families (one buffer, ii | ig | gg)
__global__ __launch_bounds__(256) void k_bj_gather(long long cnt, const int *__restrict__ map, const double *__restrict__ nzval,
                                                   double *__restrict__ vals) {
  for (long long k = blockIdx.x * 256ll + threadIdx.x; k < cnt; k += (long long)gridDim.x * 256) vals[k] = nzval[map[k]];
}
// flag[0] = 1 when a diagonal entry of a kept inverse (blockIdx.x < nsteps: the level of that step) or of S_G^-1
// (blockIdx.x == nsteps) is not positive and finite: inverses of SPD matrices are SPD
__global__ __launch_bounds__(256) void k_bj_check(int nsteps, int ndom, const GjStep *__restrict__ steps, const GjDom *__restrict__ doms,
                                                  const double *__restrict__ zstore, const double *__restrict__ sinv, int *__restrict__ flag) {
  const double *Z;
  int n;
  if ((int)blockIdx.x < nsteps) {
    const GjStep st = steps[(size_t)blockIdx.x * ndom + blockIdx.z];
    Z = zstore + st.zoff; n = st.n0;
  } else {
    const GjDom dm = doms[blockIdx.z];
    Z = sinv + dm.s_off; n = dm.ng;
  }
  for (int i = threadIdx.x; i < n; i += 256) {
    const double v = Z[i + (size_t)i * n];
    if (!(isfinite(v) && v > 0.0)) flag[0] = 1;
  }
}
// y = Z_0 g_0 (the level of the last step: every block reaches level 0 there)
__global__ __launch_bounds__(256) void k_bj_zg0(int step, int ndom, const GjStep *__restrict__ steps, const GjDom *__restrict__ doms,
                                                const double *__restrict__ zstore, const double *__restrict__ gstore, const int *done) {
  if (done && *done) return;
  const GjStep st = steps[(size_t)step * ndom + blockIdx.z];
  if (st.n0 == 0 || (int)blockIdx.x * 64 >= st.n0) return;
  gj_gemv64(zstore + st.zoff, st.n0, gstore + st.b_off, doms[blockIdx.z].y);
}
// u_G = S_G^-1 (r_G - B' y): one workgroup per 64 rows of S_G^-1, the block in blockIdx.z. t_G is formed in LDS by every
// workgroup (all of them need all of it): per seed, its column of B in stored order summed from 0, then subtracted.
__global__ __launch_bounds__(256) void k_bj_gamma(int ndom, const GjDom *__restrict__ doms, const int *__restrict__ c_ptr,
                                                  const int *__restrict__ c_row, const int *__restrict__ c_src, const double *__restrict__ ig_val,
                                                  const int *__restrict__ pos_g, const double *__restrict__ r, const double *__restrict__ sinv,
                                                  double *__restrict__ u_g, const int *done) {
  if (done && *done) return;
  const GjDom dm = doms[blockIdx.z];
  const int n = dm.ng;
  if (n == 0 || (int)blockIdx.x * 64 >= n) return;
  __shared__ double t[LV_MAX];
  __shared__ double part[4][64];
  const int *cp = c_ptr + dm.bptr;
  const int *pg = pos_g + dm.w_off;
  for (int i = threadIdx.x; i < n; i += 256) {
    double v = r[pg[i]];
    if (dm.n_last > 0) {
      double s2 = 0.0;
      for (int p = cp[i]; p < cp[i + 1]; ++p) s2 += ig_val[c_src[p]] * dm.y[c_row[p]];
      v -= s2;
    }
    t[i] = v;
  }
  __syncthreads();
  lv_gemv64_lds(sinv + dm.s_off, n, t, part, u_g + dm.w_off);
}
// u_0 = Z_0 (g_0 - B u_G): k_lv_back at level 0, the operand from the ROW form of B (ascending seed) and u_G
__global__ __launch_bounds__(256) void k_bj_back0(int step, int ndom, const GjStep *__restrict__ steps, const GjDom *__restrict__ doms,
                                                  const double *__restrict__ zstore, const double *__restrict__ gstore,
                                                  const int *__restrict__ b_off, const int *__restrict__ b_ptr, const int *__restrict__ b_col,
                                                  const int *__restrict__ b_src, const double *__restrict__ ig_val,
                                                  const double *__restrict__ u_g, double *__restrict__ ustore, const int *done) {
  if (done && *done) return;
  const GjStep st = steps[(size_t)step * ndom + blockIdx.z];
  const int n = st.n0;
  if (n == 0 || (int)blockIdx.x * 64 >= n) return;
  __shared__ double t[LV_MAX];
  __shared__ double part[4][64];
  const double *g = gstore + st.b_off;
  const double *ug = u_g + doms[blockIdx.z].w_off;
  const int *rp = b_ptr + b_off[blockIdx.z];
  for (int i = threadIdx.x; i < n; i += 256) {
    double s2 = 0.0;
    for (int p = rp[i]; p < rp[i + 1]; ++p) s2 += ig_val[b_src[p]] * ug[b_col[p]];
    t[i] = g[i] - s2;
  }
  __syncthreads();
  lv_gemv64_lds(zstore + st.zoff, n, t, part, ustore + st.b_off);
}
// z[row] = u for the level nodes (ustore, level order) and the seeds (u_G) in one launch
__global__ __launch_bounds__(256) void k_bj_scatter(long long n_i, long long n_g, const int *__restrict__ perm, const int *__restrict__ pos_g,
                                                    const double *__restrict__ ustore, const double *__restrict__ u_g, double *__restrict__ z,
                                                    const int *done) {
  if (done && *done) return;
  for (long long q = blockIdx.x * 256ll + threadIdx.x; q < n_i + n_g; q += (long long)gridDim.x * 256) {
    if (q < n_i) z[perm[q]] = ustore[q];
    else z[pos_g[q - n_i]] = u_g[q - n_i];
  }
}
#pragma clang fp contract(off)

struct BlockJacobiOp : Operator {
  bj::Split sp;
  std::unique_ptr<mi_setup_s> plan;                     // owned: the levels of every block, kept
  int nb = 0, step_dom = 0;                             // step_dom: the step whose levels hold the most entries
  long long n_i = 0, n_g = 0, n_val = 0, off_ig = 0, off_gg = 0, nnz = 0;
  int64_t kept = 0, sg = 0, dom_bytes = 0;              // 8 Σ n_k², 8 Σ n_G², 8 Σ n_k² of step_dom
  std::vector<int64_t> ng_h;
  DevBuf<int> map, perm, pos_g, b_off, b_ptr, b_col, b_src, flag;
  DevBuf<double> vals, cand, sinv, sinv_c, Sd, u_g, stage;
  bool factored = false;                                // false only inside the constructor's first factor()

  BlockJacobiOp(mi_ctx_s *c, int64_t n_, const int64_t *colptr, const int64_t *rowval, const double *nzval, int64_t nb_,
                const int64_t *seed_ptr, const int64_t *seed_idx, int base)
      : Operator(c, n_) {
    const char *me = "mi_block_jacobi_create";
    if (c->n_ranks > 1) raise(MI_ERR_BAD_ARG, "%s: the operator is replicated only; this context is rank %d of %d", me, c->rank, c->n_ranks);
    if (n_ <= 0 || n_ >= INT32_MAX || !colptr || !nzval || (base != 0 && base != 1) || (seed_ptr && !seed_idx))
      raise(MI_ERR_BAD_ARG, "%s: bad n = %lld, NULL colptr / nzval / seed_idx or index_base = %d", me, (long long)n_, base);
    if (colptr[0] != base) raise(MI_ERR_BAD_ARG, "%s: colptr[0] = %lld is not index_base = %d", me, (long long)colptr[0], base);
    nnz = colptr[n_] - base;
    if (nnz < 0 || nnz >= INT32_MAX || (nnz && !rowval)) raise(MI_ERR_BAD_ARG, "%s: bad nnz = %lld or NULL rowval", me, nnz);
    if (nb_ < 1 || nb_ > n_) raise(MI_ERR_BAD_ARG, "%s: nb = %lld blocks for n = %lld rows (1 <= nb <= n)", me, (long long)nb_, (long long)n_);
    if (nb_ > GJ_MAX_DOM) raise(MI_ERR_BAD_ARG, "%s: nb = %lld blocks, at most %d", me, (long long)nb_, GJ_MAX_DOM);
    nb = (int)nb_;
    {
      std::vector<int64_t> cp((size_t)n_ + 1), rv((size_t)nnz), sq, sx;
      for (int64_t k = 0; k <= n_; ++k) cp[k] = colptr[k] - base;
      for (int64_t k = 0; k < nnz; ++k) rv[k] = rowval[k] - base;
      if (seed_ptr) {
        if (seed_ptr[0] != base) raise(MI_ERR_BAD_ARG, "%s: seed_ptr[0] = %lld is not index_base = %d", me, (long long)seed_ptr[0], base);
        for (int d = 0; d < nb; ++d)
          if (seed_ptr[d + 1] < seed_ptr[d]) raise(MI_ERR_BAD_ARG, "%s: seed_ptr decreases at block %d (%lld after %lld)", me, d + base,
                                                   (long long)seed_ptr[d + 1], (long long)seed_ptr[d]);
        sq.resize((size_t)nb + 1);
        for (int d = 0; d <= nb; ++d) sq[d] = seed_ptr[d] - base;
        for (int64_t q = 0; q < sq[nb]; ++q) sx.push_back(seed_idx[q] - base);
      }
      std::string err;
      if (!bj::make_split(n_, cp.data(), rv.data(), nb_, seed_ptr ? sq.data() : nullptr, sx.data(), base, sp, err))
        raise(MI_ERR_BAD_ARG, "%s: %s", me, err.c_str());
    }
    std::vector<int64_t> ni_h(nb);
    ng_h.resize(nb);
    std::vector<const int64_t *> p_ii(nb), x_ii(nb), p_ig(nb), x_ig(nb), p_gg(nb), x_gg(nb);
    static const int64_t none = 0;
    for (int d = 0; d < nb; ++d) {
      ng_h[d] = (int64_t)sp.G[d].size(); ni_h[d] = (int64_t)sp.I[d].size();
      if (ng_h[d] > LV_MAX)
        raise(MI_ERR_BAD_ARG, "%s: block %d has %lld seeds, the Γ kernel stages at most %d", me, d + base, (long long)ng_h[d], LV_MAX);
      auto at = [](const std::vector<int64_t> &v) { return v.empty() ? &none : v.data(); };
      p_ii[d] = sp.ii_ptr[d].data(); x_ii[d] = at(sp.ii_idx[d]); p_ig[d] = sp.ig_ptr[d].data(); x_ig[d] = at(sp.ig_idx[d]);
      p_gg[d] = sp.gg_ptr[d].data(); x_gg[d] = at(sp.gg_idx[d]);
    }
    plan.reset(new mi_setup_s);
    setup_plan_build(*plan, c, nb, ng_h.data(), ni_h.data(), p_ii.data(), x_ii.data(), p_ig.data(), x_ig.data(), p_gg.data(), x_gg.data(), 0);
    for (int d = 0; d < nb; ++d)
      if (plan->dom[d].max_lev > LV_MAX)
        raise(MI_ERR_BAD_ARG, "%s: block %d has a level of %d nodes, the back-substitution kernel stages at most %d", me, d + base,
              plan->dom[d].max_lev, LV_MAX);
    gj_set_keep(*plan, true);
    n_i = plan->n_bi; n_g = plan->n_w;
    off_ig = plan->n_ii; off_gg = off_ig + plan->n_ig; n_val = off_gg + plan->n_gg;
    hipStream_t s = c->stream;
    // perm ∘ pos: position in level order -> row of A; seeds -> row of A
    std::vector<int> hp((size_t)n_i), pos_i((size_t)n_i), hg((size_t)n_g);
    if (n_i) memcpy_sync(hp.data(), plan->perm.p, sizeof(int) * (size_t)n_i, hipMemcpyDeviceToHost);
    {
      size_t qi = 0, qg = 0;
      for (int d = 0; d < nb; ++d) {
        for (int v : sp.I[d]) pos_i[qi++] = sp.lo[d] + v;
        for (int v : sp.G[d]) hg[qg++] = sp.lo[d] + v;
      }
    }
    for (auto &v : hp) v = pos_i[(size_t)v];
    // row form of B = B[L_0, G] per block, from the plan's column form: the entries of a row in ascending seed
    std::vector<int> bo(nb), bp, bc, bs;
    const GjState &G = *plan->gj;
    for (int d = 0; d < nb; ++d) {
      const SetupDom &D = plan->dom[d];
      bo[d] = (int)bp.size();
      setup::row_form(D.nlev ? D.lev_off[1] : 0, D.n_g, plan->c_ptr_h.data() + D.bptr_off, plan->c_row_h.data(), plan->c_src_h.data(), bp, bc, bs);
      for (int k = 0; k < D.nlev; ++k) { const int64_t w = D.lev_off[k + 1] - D.lev_off[k]; kept += 8 * w * w; }
      sg += 8 * ng_h[d] * ng_h[d];
    }
    for (int st = 0; st < G.nsteps; ++st) {
      int64_t b = 0;
      for (int d = 0; d < nb; ++d) { const int64_t w = G.steps_h[(size_t)st * nb + d].n0; b += 8 * w * w; }
      if (b > dom_bytes) { dom_bytes = b; step_dom = st; }
    }
    std::vector<int> hm;
    hm.reserve((size_t)n_val);
    hm.insert(hm.end(), sp.map_ii.begin(), sp.map_ii.end());
    hm.insert(hm.end(), sp.map_ig.begin(), sp.map_ig.end());
    hm.insert(hm.end(), sp.map_gg.begin(), sp.map_gg.end());
    auto up = [&](DevBuf<int> &dst, const std::vector<int> &h) { dst.upload(h.empty() ? std::vector<int>{0} : h, s); };
    up(map, hm); up(perm, hp); up(pos_g, hg); up(b_off, bo); up(b_ptr, bp); up(b_col, bc); up(b_src, bs);
    vals.alloc((size_t)n_val + 1); cand.alloc((size_t)n_val + 1);
    sinv.alloc((size_t)plan->n_s + 1); sinv_c.alloc((size_t)plan->n_s + 1); Sd.alloc((size_t)plan->n_s + 1);
    u_g.alloc((size_t)n_g + 1);
    flag.alloc(1);
    {
      DevBuf<double> v;
      v.upload(nzval, (size_t)nnz, s);
      factor(v.p);
    }
    MI_HIP(hipStreamSynchronize(s));
  }

  void run(const double *v) { gj_run(*plan, v, v + off_ig, v + off_gg, nullptr, Sd.p, nullptr); }

  // The numeric phase on device values `nz` (the CSC order of create). Synchronous; raises MI_ERR_SINGULAR and keeps the
  // previous factor: the kept levels are the plan's, so they are restored by a run on the accepted values (every sum of
  // the elimination has a fixed order: the same bits come back).
  void factor(const double *nz) {
    hipStream_t s = ctx->stream;
    GjState &G = *plan->gj;
    if (n_val) hipLaunchKernelGGL(k_bj_gather, dim3(grid_for(n_val)), dim3(256), 0, s, n_val, (const int *)map.p, nz, cand.p);
    MI_HIP(hipGetLastError());
    try {
      run(cand.p);
      pinv_blocks_fast(ctx, nb, ng_h.data(), Sd.p, 0.0, sinv_c.p, true);
      MI_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), s));
      hipLaunchKernelGGL(k_bj_check, dim3(G.nsteps + 1, 1, nb), dim3(256), 0, s, G.nsteps, nb, (const GjStep *)G.steps.p, (const GjDom *)G.doms.p,
                         (const double *)G.zstore.p, (const double *)sinv_c.p, flag.p);
      MI_HIP(hipGetLastError());
      int fh = 0;
      MI_HIP(hipMemcpyAsync(&fh, flag.p, sizeof fh, hipMemcpyDeviceToHost, s));
      MI_HIP(hipStreamSynchronize(s));
      if (fh) raise(MI_ERR_SINGULAR, "mi_block_jacobi: a diagonal block is singular or not positive definite (a kept inverse has a diagonal entry that is not positive)");
    } catch (const Error &e) {
      if (e.code != MI_ERR_SINGULAR) throw;
      const std::string msg = last_error();
      (void)hipStreamSynchronize(s);
      if (factored) { run(vals.p); MI_HIP(hipStreamSynchronize(s)); }
      raise(MI_ERR_SINGULAR, "%s", msg.rfind("mi_block_jacobi", 0) == 0 ? msg.c_str() : ("mi_block_jacobi: " + msg).c_str());
    }
    // accepted: into the live buffers (same addresses, so captured solve graphs stay valid)
    if (n_val) MI_HIP(hipMemcpyAsync(vals.p, cand.p, sizeof(double) * (size_t)n_val, hipMemcpyDeviceToDevice, s));
    if (plan->n_s) MI_HIP(hipMemcpyAsync(sinv.p, sinv_c.p, sizeof(double) * (size_t)plan->n_s, hipMemcpyDeviceToDevice, s));
    MI_HIP(hipStreamSynchronize(s));
    factored = true;
  }

  void apply(const double *x, double *z, const int *done) override {
    hipStream_t s = ctx->stream;
    GjState &G = *plan->gj;
    const GjStep *st = G.steps.p;
    const GjDom *dm = G.doms.p;
    auto cdiv = [](int a, int b) { return (a + b - 1) / b; };
    const int S = G.nsteps, ngm = std::max(1, G.ngmax);
    const double *ig = vals.p + off_ig;
    gj_level_forward(*plan, s, perm.p, x, done);
    if (S > 0)
      hipLaunchKernelGGL(k_bj_zg0, dim3(cdiv(G.n_step[S - 1], 64), 1, nb), dim3(256), 0, s, S - 1, nb, st, dm, (const double *)G.zstore.p,
                         (const double *)G.gstore.p, done);
    hipLaunchKernelGGL(k_bj_gamma, dim3(cdiv(ngm, 64), 1, nb), dim3(256), 0, s, nb, dm, (const int *)plan->c_ptr.p, (const int *)plan->c_row.p,
                       (const int *)plan->c_src.p, ig, (const int *)pos_g.p, x, (const double *)sinv.p, u_g.p, done);
    if (S > 0) {
      hipLaunchKernelGGL(k_bj_back0, dim3(cdiv(G.n_step[S - 1], 64), 1, nb), dim3(256), 0, s, S - 1, nb, st, dm, (const double *)G.zstore.p,
                         (const double *)G.gstore.p, (const int *)b_off.p, (const int *)b_ptr.p, (const int *)b_col.p, (const int *)b_src.p, ig,
                         (const double *)u_g.p, G.ustore.p, done);
      gj_level_backward(*plan, s, S - 2, done);
    }
    hipLaunchKernelGGL(k_bj_scatter, dim3(grid_for(n)), dim3(256), 0, s, n_i, n_g, (const int *)perm.p, (const int *)pos_g.p,
                       (const double *)G.ustore.p, (const double *)u_g.p, z, done);
    MI_HIP(hipGetLastError());
  }
  // bytes of one apply: every kept inverse twice, S_G^-1 once, and per node the vectors and maps of the launches above —
  // a level node: r, g (written, read by the product and by the back-substitution), y (written, read), u (written, read by
  // the next level and by the scatter), z: 10 doubles and perm twice; a seed: r, u_G (written, read by level 0 and by the
  // scatter), z: 5 doubles and pos_g twice. The sparse coupling entries (16 bytes each, read twice) are not counted.
  // Dominant: the back-substitution launch of the step whose levels hold the most entries.
  void bytes(int64_t *a, int64_t *d) const override {
    *a = 2 * kept + sg + 88 * (int64_t)n_i + 48 * (int64_t)n_g;
    *d = dom_bytes;
  }
  void apply_dominant(const double *x) override {
    GjState &G = *plan->gj;
    if (!factored || G.nsteps == 0) return;
    hipLaunchKernelGGL(k_lv_back, dim3((G.n_step[step_dom] + 63) / 64, 1, nb), dim3(256), 0, ctx->stream, step_dom, 1, nb, (const GjStep *)G.steps.p,
                       (const double *)G.zstore.p, (const double *)G.gstore.p, (const int *)G.r_ptr.p, (const int *)G.r_col.p, (const int *)G.r_src.p,
                       (const double *)G.in_ii.p, G.ustore.p, (const int *)nullptr);
  }
};

}  // namespace mi
#endif   // __HIPCC__
