// Smoothed-aggregation AMG preconditioner on the full system: the reference's `AMGPreconditioner{SmoothedAggregation}(A)`
// (Preconditioners.jl), the M of `pcg(A, b, 0, Π_amg)` in Example01:49-61 / Example10 and of Examples 06, 09, 12-20.
// The hierarchy (A_l, P_l, ω_l / diag(A_l), the dense inverse of the coarsest level) is built on the host once per matrix
// (fem.prepare_amg_precond), or its numbers are redone on the device for every new realization on frozen aggregates
// (amg_setup.hpp, mi_amg_plan_create / mi_amg_set_values); this file holds the V(1,1) cycle. Deviation from the reference: its smoother is symmetric
// Gauss-Seidel, a sequential sweep with no bit-reproducible device form; here one pre- and one post-sweep of Jacobi damped
// by ω_l = 4 / (3 g_l), g_l the Gershgorin bound on ρ(D^-1 A_l) — the cycle is symmetric, so M is SPD.
//
//   cycle(l, b):   coarsest: x = A_c^-1 b                                   k_amg_coarse (dense GEMV, one wave per row)
//     x = (ω/d) b;  r = b - A_l x                                            k_amg_down     one pass over A_l
//     b_{l+1} = R_l r,  R_l = P_l' in CSR (a row gather, not a scatter)      k_amg_restrict
//     e = cycle(l + 1, b_{l+1})
//     x += P_l e                                                             k_amg_prolong
//     x_new = x + (ω/d) (b - A_l x)      out of place                        k_amg_post
//
// 4 (nlevels - 1) + 1 launches on the context's stream, no atomics, no host synchronisation, every launch honours `done`.
// All four sparse kernels are the CSR-stream form of k_spmv_csr on the row blocks of spmv_blocks.hpp: products parked in
// LDS, each row summed left to right in CSR order by one thread, no contraction — two applies give the same bits. No kernel
// reads a word that another workgroup of the same launch writes (k_amg_down gathers ω/d · b, never the x it stores;
// k_amg_prolong updates x[r] in the thread that read it and gathers e only).
#pragma once
#include "operators.hpp"

namespace mi {

constexpr int AMG_MAX_COARSE = 4096;   // rows of the dense coarsest inverse (fem.AMG_MAX_COARSE_ROWS)

// Row sums of one row block: prod[k] = val[k] * gather(col[k]) in LDS, then out(r, Σ_k prod[k]) per row, k ascending.
// A single row longer than the tile: tile by tile, thread 0 keeps the running left-to-right sum (as k_spmv_csr).
template <class G, class O>
__device__ __forceinline__ void amg_block_rows(int nblocks, const SpmvBlock *__restrict__ blk, const int *__restrict__ rowptr,
                                               const int *__restrict__ col, const double *__restrict__ val, double *prod, G gather, O out) {
  const int per = (nblocks + 7) >> 3;
  const int b = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);   // contiguous block ranges per XCD (k_spmv_csr)
  if (b >= nblocks) return;
  const SpmvBlock bi = blk[b];
  const int r0 = bi.r0, r1 = bi.r1, k0 = bi.k0;
  const int nnz = bi.k1 - k0;
  if (nnz <= SPMV_TILE) {
    if ((k0 & 1) == 0) {   // 16-byte aligned values, 8-byte aligned indices: two non-zeros per load
      const int npair = (nnz + 1) >> 1;
      for (int q = threadIdx.x; q < npair; q += NT) {
        const int k = 2 * q;
        if (k + 1 < nnz) {
          const int2 c = *reinterpret_cast<const int2 *>(col + k0 + k);
          const double2 v = *reinterpret_cast<const double2 *>(val + k0 + k);
          *reinterpret_cast<double2 *>(&prod[k]) = make_double2(v.x * gather(c.x), v.y * gather(c.y));
        } else {
          prod[k] = val[k0 + k] * gather(col[k0 + k]);
        }
      }
    } else {
      for (int k = threadIdx.x; k < nnz; k += NT) prod[k] = val[k0 + k] * gather(col[k0 + k]);
    }
    __syncthreads();
    for (int r = r0 + threadIdx.x; r < r1; r += NT) {
      const int a = rowptr[r] - k0, e = rowptr[r + 1] - k0;
      double sum = 0.0;
      for (int k = a; k < e; ++k) sum += prod[k];
      out(r, sum);
    }
  } else {
    double sum = 0.0;
    for (int t0 = 0; t0 < nnz; t0 += SPMV_TILE) {
      const int m = min(SPMV_TILE, nnz - t0);
      for (int k = threadIdx.x; k < m; k += NT) prod[k] = val[k0 + t0 + k] * gather(col[k0 + t0 + k]);
      __syncthreads();
      if (threadIdx.x == 0)
        for (int k = 0; k < m; ++k) sum += prod[k];
      __syncthreads();
    }
    if (threadIdx.x == 0) out(r0, sum);
  }
}

#define MI_AMG_CSR_ARGS int nblocks, const SpmvBlock *__restrict__ blk, const int *__restrict__ rowptr, const int *__restrict__ col, \
                        const double *__restrict__ val
// x = (ω/d) b and r = b - A x in one pass over A: the gathered operand is (ω/d)_j b_j, formed on the fly
__global__ __launch_bounds__(NT) void k_amg_down(MI_AMG_CSR_ARGS, const double *__restrict__ wd, const double *__restrict__ b,
                                                 double *__restrict__ x, double *__restrict__ r, const int *done) {
  if (done && *done) return;
  __shared__ __attribute__((aligned(16))) double prod[SPMV_TILE];
  amg_block_rows(nblocks, blk, rowptr, col, val, prod, [&](int c) { return wd[c] * b[c]; },
                 [&](int i, double s) { const double bi = b[i]; x[i] = wd[i] * bi; r[i] = bi - s; });
}
// y = R v
__global__ __launch_bounds__(NT) void k_amg_restrict(MI_AMG_CSR_ARGS, const double *__restrict__ v, double *__restrict__ y, const int *done) {
  if (done && *done) return;
  __shared__ __attribute__((aligned(16))) double prod[SPMV_TILE];
  amg_block_rows(nblocks, blk, rowptr, col, val, prod, [&](int c) { return v[c]; }, [&](int i, double s) { y[i] = s; });
}
// x += P e
__global__ __launch_bounds__(NT) void k_amg_prolong(MI_AMG_CSR_ARGS, const double *__restrict__ e, double *x, const int *done) {
  if (done && *done) return;
  __shared__ __attribute__((aligned(16))) double prod[SPMV_TILE];
  amg_block_rows(nblocks, blk, rowptr, col, val, prod, [&](int c) { return e[c]; }, [&](int i, double s) { x[i] = x[i] + s; });
}
// y = x + (ω/d) (b - A x), y != x
__global__ __launch_bounds__(NT) void k_amg_post(MI_AMG_CSR_ARGS, const double *__restrict__ wd, const double *__restrict__ b,
                                                 const double *__restrict__ x, double *__restrict__ y, const int *done) {
  if (done && *done) return;
  __shared__ __attribute__((aligned(16))) double prod[SPMV_TILE];
  amg_block_rows(nblocks, blk, rowptr, col, val, prod, [&](int c) { return x[c]; },
                 [&](int i, double s) { y[i] = x[i] + wd[i] * (b[i] - s); });
}
// the level-0 post-smoothing of a cycle inside the interior CG (interior_amg.hpp): as k_amg_post, and the row epilogue also
// sums b_i y_i = r_i z_i over the rows of the block, thread by thread in ascending row, then the fixed tree of block_sum:
// part[block]. The row blocks are cut at subdomain boundaries, so a subdomain's r'z is a run of these partials.
__global__ __launch_bounds__(NT) void k_amg_post_dot(MI_AMG_CSR_ARGS, const double *__restrict__ wd, const double *__restrict__ b,
                                                     const double *__restrict__ x, double *__restrict__ y, double *__restrict__ part,
                                                     const int *done) {
  if (done && *done) return;
  __shared__ __attribute__((aligned(16))) double prod[SPMV_TILE];
  __shared__ double sm[NT / 64 + 1];
  double by = 0.0;
  amg_block_rows(nblocks, blk, rowptr, col, val, prod, [&](int c) { return x[c]; },
                 [&](int i, double s) { const double bi = b[i], yi = x[i] + wd[i] * (bi - s); y[i] = yi; by += bi * yi; });
  const int bl = (int)(blockIdx.x & 7) * ((nblocks + 7) >> 3) + (int)(blockIdx.x >> 3);   // the block amg_block_rows worked on
  if (bl >= nblocks) return;
  by = block_sum(by, sm);
  if (threadIdx.x == 0) part[bl] = by;
}
#undef MI_AMG_CSR_ARGS
// y = Z b for the symmetric n x n inverse of the coarsest level (column j of the column-major Z is its row j): one wave per
// row, lane q sums the columns q, q + 64, ... in ascending order, then the fixed shuffle tree.
__global__ __launch_bounds__(NT) void k_amg_coarse(int n, const double *__restrict__ Z, const double *__restrict__ b, double *__restrict__ y,
                                                   const int *done) {
  if (done && *done) return;
  const int row = (int)blockIdx.x * (NT / 64) + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n) return;
  const double *z = Z + (size_t)row * n;
  double s = 0.0;
  for (int j = lane; j < n; j += 64) s += z[j] * b[j];
  s = wave_sum(s);
  if (lane == 0) y[row] = s;
}

// The same for the inverse of a block-diagonal coarsest level (the stacked A_II of the interior CG): row i takes the columns
// of its own subdomain only, dom[j] == dom[i]. The entries left out are the zeros of the inverse, and a value that is not
// finite in one subdomain's right-hand side stays in that subdomain. With `rz`: rz[i] = b_i y_i (a one-level hierarchy has
// no post-smoothing launch to leave the partials of r'z; the interior CG then sums these row by row).
__global__ __launch_bounds__(NT) void k_amg_coarse_dom(int n, const double *__restrict__ Z, const int *__restrict__ dom, const double *__restrict__ b,
                                                       double *__restrict__ y, double *__restrict__ rz, const int *done) {
  if (done && *done) return;
  const int row = (int)blockIdx.x * (NT / 64) + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n) return;
  const double *z = Z + (size_t)row * n;
  const int dr = dom[row];
  double s = 0.0;
  for (int j = lane; j < n; j += 64)
    if (dom[j] == dr) s += z[j] * b[j];
  s = wave_sum(s);
  if (lane == 0) { y[row] = s; if (rz) rz[row] = b[row] * s; }
}

struct AmgOp : Operator {
  struct Level {
    CsrDev A, P, R;          // P, R = P' and the smoother only below the coarsest level
    DevBuf<double> wd;       // ω_l / diag(A_l)
    DevBuf<double> b, x, r, y;   // level vectors: right-hand side (l > 0), iterate, residual, post-smoothed iterate (l > 0; coarsest: the solution)
    int n = 0;
  };
  std::vector<Level> lv;
  DevBuf<double> zinv, sink_x, sink_r;
  DevBuf<int> coarse_dom;   // interior_amg.hpp: the subdomain of every row of the coarsest level (empty: one dense inverse)
  int nlev = 0, nc = 0;
  int64_t op_nnz = 0, kept = 0, alg = 0, dom = 0;
  HostCsr coarse_h;   // A of the coarsest level as given (the cycle needs only its inverse): read back by mi_amg_level_get
  std::vector<double> omega_h;   // ω_l of the smoothed levels, for the read-back. mi_amg_create is given ω/d only: there ω_l is
                                 // recovered as (ω/d)_0 a_00, one rounding away (NaN without a stored a_00)

  // Read-back of one level (mi_amg_level_sizes / mi_amg_level_get): HOST arrays, 0-based, any pointer may be NULL.
  void level_sizes(int l, int64_t *nr, int64_t *ncol, int64_t *a_nnz, int64_t *p_nnz) const {
    const Level &L = lv[(size_t)l];
    const bool host_a = l == nlev - 1 && L.A.n_rows == 0;
    if (nr) *nr = L.n;
    if (ncol) *ncol = l < nlev - 1 ? lv[(size_t)l + 1].n : 0;
    if (a_nnz) *a_nnz = host_a ? coarse_h.nnz() : L.A.nnz;
    if (p_nnz) *p_nnz = l < nlev - 1 ? L.P.nnz : 0;
  }
  void level_get(int l, int64_t *a_ptr, int64_t *a_col, double *a_val, int64_t *p_ptr, int64_t *p_col, double *p_val, double *omega, double *wd_out) {
    hipStream_t s = ctx->stream;
    Level &L = lv[(size_t)l];
    auto ints = [&](const int *dev, size_t cnt, int64_t *out) {
      if (!out || !cnt) return;
      std::vector<int> h(cnt);
      MI_HIP(hipMemcpyAsync(h.data(), dev, cnt * sizeof(int), hipMemcpyDeviceToHost, s));
      MI_HIP(hipStreamSynchronize(s));
      for (size_t k = 0; k < cnt; ++k) out[k] = h[k];
    };
    auto vals = [&](const double *dev, size_t cnt, double *out) {
      if (!out || !cnt) return;
      MI_HIP(hipMemcpyAsync(out, dev, cnt * sizeof(double), hipMemcpyDeviceToHost, s));
      MI_HIP(hipStreamSynchronize(s));
    };
    auto csr = [&](const CsrDev &M, int64_t *ptr, int64_t *col, double *val) {
      ints(M.rowptr.p, (size_t)M.n_rows + 1, ptr); ints(M.col.p, (size_t)M.nnz, col); vals(M.val.p, (size_t)M.nnz, val);
    };
    if (l == nlev - 1 && L.A.n_rows == 0) {
      if (a_ptr) std::copy(coarse_h.rowptr.begin(), coarse_h.rowptr.end(), a_ptr);
      if (a_col) std::copy(coarse_h.col.begin(), coarse_h.col.end(), a_col);
      if (a_val) std::copy(coarse_h.val.begin(), coarse_h.val.end(), a_val);
    } else csr(L.A, a_ptr, a_col, a_val);
    if (l == nlev - 1) return;
    csr(L.P, p_ptr, p_col, p_val);
    if (omega) *omega = omega_h[(size_t)l];
    vals(L.wd.p, (size_t)L.n, wd_out);
  }

  // for amg_setup.hpp (mi_amg_plan_create), which fills the levels itself
  AmgOp(mi_ctx_s *c, int64_t n0) : Operator(c, n0) {}

  static void check_finite(const char *me, const char *what, int l, const double *v, size_t cnt) {
    for (size_t k = 0; k < cnt; ++k)
      if (!std::isfinite(v[k])) raise(MI_ERR_BAD_ARG, "%s: %s of level %d holds %g at entry %zu (not finite)", me, what, l, v[k], k);
  }

  AmgOp(mi_ctx_s *c, int64_t nlevels, const int64_t *n_l, const int64_t *const *a_rowptr, const int64_t *const *a_colidx,
        const double *const *a_val, const int64_t *const *p_rowptr, const int64_t *const *p_colidx, const double *const *p_val,
        const double *omega_over_d, const double *coarse_inv, int base)
      : Operator(c, n_l[0]) {
    const char *me = "mi_amg_create";
    if (c->n_ranks > 1) raise(MI_ERR_BAD_ARG, "%s: the operator is replicated only; this context is rank %d of %d", me, c->rank, c->n_ranks);
    if (base != 0 && base != 1) raise(MI_ERR_BAD_ARG, "%s: index_base = %d (0 or 1)", me, base);
    if (!a_rowptr || !a_colidx || !a_val || !coarse_inv || (nlevels > 1 && (!p_rowptr || !p_colidx || !p_val || !omega_over_d)))
      raise(MI_ERR_BAD_ARG, "%s: NULL array of level arrays, omega_over_d or coarse_inv", me);
    for (int64_t l = 0; l < nlevels; ++l) {
      if (n_l[l] < 1 || n_l[l] >= INT32_MAX) raise(MI_ERR_BAD_ARG, "%s: level %lld has n = %lld rows", me, (long long)l, (long long)n_l[l]);
      if (l && n_l[l] >= n_l[l - 1])
        raise(MI_ERR_BAD_ARG, "%s: the level sizes do not chain: level %lld has %lld rows after %lld", me, (long long)l, (long long)n_l[l],
              (long long)n_l[l - 1]);
    }
    nlev = (int)nlevels; nc = (int)n_l[nlevels - 1];
    if (nc > AMG_MAX_COARSE) raise(MI_ERR_BAD_ARG, "%s: the coarsest level has %d rows, the dense inverse holds at most %d", me, nc, AMG_MAX_COARSE);
    hipStream_t s = c->stream;
    lv.resize((size_t)nlev);
    size_t woff = 0;
    for (int l = 0; l < nlev; ++l) {
      Level &L = lv[(size_t)l];
      L.n = (int)n_l[l];
      if (!a_rowptr[l]) raise(MI_ERR_BAD_ARG, "%s: A of level %d is NULL", me, l);
      const HostCsr ha = host_csr(L.n, L.n, a_rowptr[l], a_colidx[l], a_val[l], base);
      check_finite(me, "A", l, ha.val.data(), ha.val.size());
      op_nnz += ha.nnz();
      if (l == nlev - 1) { coarse_h = ha; break; }
      const int n1 = (int)n_l[l + 1];
      if (!p_rowptr[l]) raise(MI_ERR_BAD_ARG, "%s: P of level %d is NULL", me, l);
      HostCsr hp;
      try {
        hp = host_csr(L.n, n1, p_rowptr[l], p_colidx[l], p_val[l], base);
      } catch (const Error &e) {
        const std::string why = last_error();
        raise(e.code, "%s: P of level %d is not %d x %d: %s", me, l, L.n, n1, why.c_str());
      }
      check_finite(me, "P", l, hp.val.data(), hp.val.size());
      check_finite(me, "omega_over_d", l, omega_over_d + woff, (size_t)L.n);
      L.A.upload(ha, s); L.P.upload(hp, s); L.R.upload(transpose(hp), s);
      L.wd.upload(omega_over_d + woff, (size_t)L.n, s);
      {
        double a00 = std::numeric_limits<double>::quiet_NaN();
        for (int k = ha.rowptr[0]; k < ha.rowptr[1]; ++k)
          if (ha.col[(size_t)k] == 0) a00 = ha.val[(size_t)k];
        omega_h.push_back(omega_over_d[woff] * a00);
      }
      MI_HIP(hipStreamSynchronize(s));
      woff += (size_t)L.n;
      kept += 12 * ha.nnz() + 24 * hp.nnz() + 8 * (int64_t)L.n;
      alg += 2 * (12 * ha.nnz() + 4 * ((int64_t)L.n + 1)) + 24 * hp.nnz() + 4 * ((int64_t)L.n + 1) + 4 * ((int64_t)n1 + 1) + 88 * (int64_t)L.n + 16 * (int64_t)n1;
      if (l == 0) dom = 12 * ha.nnz() + 4 * ((int64_t)L.n + 1) + 32 * (int64_t)L.n;
    }
    check_finite(me, "coarse_inv", nlev - 1, coarse_inv, (size_t)nc * nc);
    zinv.upload(coarse_inv, (size_t)nc * nc, s);
    MI_HIP(hipStreamSynchronize(s));
    kept += 8 * (int64_t)nc * nc;
    alg += 8 * (int64_t)nc * nc + 16 * (int64_t)nc;
    if (nlev == 1) dom = alg;
    alloc_vectors();
  }
  // level vectors, once: nothing is allocated in apply
  void alloc_vectors() {
    for (int l = 0; l < nlev; ++l) {
      Level &L = lv[(size_t)l];
      const size_t m = (size_t)L.n + 1;
      if (l > 0) { L.b.alloc(m); L.y.alloc(m); }
      if (l < nlev - 1) { L.x.alloc(m); L.r.alloc(m); }
    }
    sink_x.alloc((size_t)n + 1); sink_r.alloc((size_t)n + 1);   // where apply_dominant writes
  }

  static int grid_of(const CsrDev &M) { return ((M.nblocks + 7) / 8) * 8; }
#define MI_AMG_CSR(M) (M).nblocks, (const SpmvBlock *)(M).blk.p, (const int *)(M).rowptr.p, (const int *)(M).col.p, (const double *)(M).val.p
  void coarse(const double *b, double *y, const int *done, double *rz = nullptr) {
    const dim3 grid((nc + NT / 64 - 1) / (NT / 64));
    if (coarse_dom.p) hipLaunchKernelGGL(k_amg_coarse_dom, grid, dim3(NT), 0, ctx->stream, nc, (const double *)zinv.p, (const int *)coarse_dom.p, b, y, rz, done);
    else hipLaunchKernelGGL(k_amg_coarse, grid, dim3(NT), 0, ctx->stream, nc, (const double *)zinv.p, b, y, done);
  }
  void apply(const double *r, double *z, const int *done) override { cycle(r, z, done, nullptr); }
  // one cycle; `rz_part` (interior_amg.hpp, needs coarse_dom): also the partials of r'z — per row block of A_0, or per row of
  // a one-level hierarchy
  void cycle(const double *r, double *z, const int *done, double *rz_part) {
    hipStream_t s = ctx->stream;
    if (nlev == 1) { coarse(r, z, done, rz_part); MI_HIP(hipGetLastError()); return; }
    for (int l = 0; l < nlev - 1; ++l) {
      Level &L = lv[(size_t)l], &N = lv[(size_t)l + 1];
      const double *b = l ? L.b.p : r;
      hipLaunchKernelGGL(k_amg_down, dim3(grid_of(L.A)), dim3(NT), 0, s, MI_AMG_CSR(L.A), (const double *)L.wd.p, b, L.x.p, L.r.p, done);
      hipLaunchKernelGGL(k_amg_restrict, dim3(grid_of(L.R)), dim3(NT), 0, s, MI_AMG_CSR(L.R), (const double *)L.r.p, N.b.p, done);
    }
    Level &C = lv[(size_t)nlev - 1];
    coarse(C.b.p, C.y.p, done);
    for (int l = nlev - 2; l >= 0; --l) {
      Level &L = lv[(size_t)l], &N = lv[(size_t)l + 1];
      const double *b = l ? L.b.p : r;
      hipLaunchKernelGGL(k_amg_prolong, dim3(grid_of(L.P)), dim3(NT), 0, s, MI_AMG_CSR(L.P), (const double *)N.y.p, L.x.p, done);
      if (l == 0 && rz_part)
        hipLaunchKernelGGL(k_amg_post_dot, dim3(grid_of(L.A)), dim3(NT), 0, s, MI_AMG_CSR(L.A), (const double *)L.wd.p, b, (const double *)L.x.p, z,
                           rz_part, done);
      else
        hipLaunchKernelGGL(k_amg_post, dim3(grid_of(L.A)), dim3(NT), 0, s, MI_AMG_CSR(L.A), (const double *)L.wd.p, b, (const double *)L.x.p,
                           l ? L.y.p : z, done);
    }
    MI_HIP(hipGetLastError());
  }
  // Algorithmic bytes of one cycle. Per smoothed level: A_l twice (12 nnz + 4 (n + 1) each), P_l and R_l once (12 nnz and
  // their row pointers), and the vectors of the four launches — down: b, ω/d, x, r; restrict: r, b_{l+1}; prolong: e, x
  // read and written; post: x, b, ω/d, the result: 11 doubles per row and 2 per coarse row. Coarsest: the inverse, b, x.
  // Dominant: the fine-level k_amg_down (A_0 once, four vectors).
  void bytes(int64_t *a, int64_t *d) const override { *a = alg; *d = dom; }
  void apply_dominant(const double *x) override {
    if (nlev == 1) { coarse(x, sink_x.p, nullptr); return; }
    Level &L = lv[0];
    hipLaunchKernelGGL(k_amg_down, dim3(grid_of(L.A)), dim3(NT), 0, ctx->stream, MI_AMG_CSR(L.A), (const double *)L.wd.p, x, sink_x.p, sink_r.p,
                       (const int *)nullptr);
  }
#undef MI_AMG_CSR
};

}  // namespace mi
