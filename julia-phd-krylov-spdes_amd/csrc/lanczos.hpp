// mi_eigsolve: extremal eigenpairs of a symmetric operator by thick-restart Lanczos with full re-orthogonalisation — for a
// symmetric operator the Hermitian Krylov-Schur method that the reference runs through KrylovKit:
//   KrylovKit.eigsolve(x -> S_local_mat*x, n_Γ, nev, :SR | :LR, krylovdim=2*nev)               Example03:209/219
//   KrylovKit.geneigsolve(x -> (S*x, A_ΓΓ*x), n_Γ, nvec, :SR, krylovdim=2*nvec, isposdef=true)  EPDD.jl:1546-1549
// and, through a user-supplied inverse operator, the `Arpack.eigs(A | S, nev, :SM)` legs (Example03:260/291/313).
//
// Standard problem A x = λ x, window m = krylovdim (clamped to n), basis V (n x (m+1)), projected matrix T (m x m):
//   step j:  w = A v_j;  h = V[:, :j+1]' w;  w -= V h;  h2 likewise (CGS2);  T[:j+1, j] = h + h2;  beta = ||w||;  v_{j+1} = w / beta
//            (projecting on ALL columns also yields the arrow-head coupling after a restart: no special case)
//   after step m-1, on the host:  T = Y Θ Y' (dense_small.hpp), ascending for SR / descending for LR;
//            rho_i = |beta Y[m-1, i]|;  nconv = leading pairs with rho_i <= tol (at most nev);
//            done if nconv >= nev, or `maxiter` restarts were made, or m == n;
//   else thick restart:  k = min(nev + (m - nev)/2, m - 1);  V[:, :k] = V[:, :m] Y[:, :k];  v_k = v_m;  T = diag(θ_1..θ_k);  go on at j = k.
// Generalized problem A x = λ B x (B SPD, given as B and as an exact B^-1): Lanczos on B^-1 A in the B inner product with a
// second panel Q = B V:  u = A v_j;  w = B^-1 u;  h = V'u;  w -= V h;  u = B w (applied, NOT the recurrence u -= Q h: that loses
// B-orthogonality steadily);  h2 = V'u;  w -= V h2;  u -= Q h2;  beta = sqrt(w'u);  v_{j+1} = w / beta;  q_{j+1} = u / beta.
// Break-down (beta <= 64 eps max|T|: V[:, :j+1] is invariant): if j + 1 >= nev the pairs of that subspace are exact and the
// call ends with m = j + 1; otherwise a fresh host-generated vector, (B-)orthogonalised twice, continues the basis. With
// m == n the last step does not normalise (its beta is rounding noise).
//
// Device / host split as for the eigCG window (eig_solvers.hpp): the panels never leave HBM; all steps from a (re)start to
// the end of the window are ONE graph replay (the active column count of every step is fixed when the graph is captured;
// break-down and non-finite flags are device state, lanczos_kernels.hpp), one host synchronisation per restart. Operators
// that are not graph_safe() run the same kernels eagerly. Every buffer and graph lives for one call: nothing is carried
// from one call to the next.
#pragma once
#include "dense_small.hpp"
#include "lanczos_kernels.hpp"
#include "operators.hpp"

namespace mi {

struct LanczosResult {
  std::vector<double> vals, resid;  // nev each
  int64_t nconv = 0, nrestart = 0, napply = 0;
};

// splitmix64 -> uniform in (-1, 1): the default start vector and the vectors that continue a broken-down basis
inline void lz_host_vector(std::vector<double> &v, unsigned long long seed) {
  unsigned long long x = 0x9E3779B97F4A7C15ull * (seed + 1);
  for (double &e : v) {
    x += 0x9E3779B97F4A7C15ull;
    unsigned long long z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    e = (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0 + 1.0 / 9007199254740992.0;
  }
}

struct Lanczos {
  mi_ctx_s *ctx;
  Operator *A, *B, *Binv;
  hipStream_t s;
  int n, g, m, nev, which;
  long long ld;
  bool gen, use_graph;
  DevBuf<double> V, Q, w, u, T, part1, part2, partn, h1, betas, tmaxs, beta0, G, Vtmp;
  DevBuf<int> status;
  std::map<int, hipGraphExec_t> graphs;  // first step -> the steps [first, m)

  Lanczos(mi_ctx_s *c, Operator *A_, Operator *B_, Operator *Binv_, int nev_, int which_, int m_)
      : ctx(c), A(A_), B(B_), Binv(Binv_), s(c->stream), n((int)A_->n), g(vec_grid(A_->n)), m(m_), nev(nev_), which(which_),
        ld(((long long)A_->n + 1) / 2 * 2), gen(B_ != nullptr) {
    use_graph = c->chunk > 0 && !c->no_graph && A->graph_safe() && (!gen || (B->graph_safe() && Binv->graph_safe()));
    const size_t panel = (size_t)ld * (m + 1);
    V.alloc(panel); w.alloc(ld);
    if (gen) { Q.alloc(panel); u.alloc(ld); }
    T.alloc((size_t)m * m); part1.alloc((size_t)m * g); part2.alloc((size_t)m * g); partn.alloc(g); h1.alloc(m);
    betas.alloc(m); tmaxs.alloc(m); beta0.alloc(1); status.alloc(m + 1); G.alloc((size_t)m * m); Vtmp.alloc((size_t)ld * m);
    // a pooled block is handed out zeroed, a fresh one is whatever the runtime gives: the padding rows must be zero
    V.zero(s); w.zero(s); Q.zero(s); u.zero(s); T.zero(s); status.zero(s); betas.zero(s); tmaxs.zero(s);
  }
  ~Lanczos() {
    for (auto &kv : graphs) (void)hipGraphExecDestroy(kv.second);
  }
  double *vcol(int j) { return V.p + (size_t)j * ld; }
  double *qcol(int j) { return gen ? Q.p + (size_t)j * ld : nullptr; }

  // CGS2 of w (u = B w) against the first ncols columns, then the norm partials. Tcol: column of T to write, or nullptr.
  void orthogonalise(int ncols, const int *stop, double *Tcol) {
    const size_t lds = lz_lds_bytes(ncols);
    hipLaunchKernelGGL(k_lz_project, dim3(g), dim3(NT), lds, s, n, ld, ncols, V.p, gen ? u.p : w.p, part1.p, stop);
    hipLaunchKernelGGL(k_lz_update_project, dim3(g), dim3(NT), lds, s, n, ld, ncols, V.p, w.p, part1.p, h1.p,
                       gen ? (double *)nullptr : part2.p, stop);
    MI_HIP(hipGetLastError());
    if (gen) {
      B->apply(w.p, u.p, stop);
      hipLaunchKernelGGL(k_lz_project, dim3(g), dim3(NT), lds, s, n, ld, ncols, V.p, u.p, part2.p, stop);
    }
    hipLaunchKernelGGL(k_lz_update_norm, dim3(g), dim3(NT), lds, s, n, ld, ncols, V.p, gen ? Q.p : (double *)nullptr, w.p,
                       gen ? u.p : (double *)nullptr, part2.p, h1.p, Tcol, partn.p, stop);
    MI_HIP(hipGetLastError());
  }
  void commit(int ncols, int dst, const double *Tcol, const int *status_in, int *status_out, double *beta_out,
              const double *tmax_prev, double *tmax_out, int mode) {
    hipLaunchKernelGGL(k_lz_commit, dim3(g), dim3(NT), 0, s, n, g, ncols, partn.p, w.p, gen ? u.p : (double *)nullptr, vcol(dst),
                       qcol(dst), Tcol, status_in, status_out, beta_out, tmax_prev, tmax_out, mode);
    MI_HIP(hipGetLastError());
  }
  void step(int j) {
    const int *stop = status.p + j;
    if (gen) {
      A->apply(vcol(j), u.p, stop);
      Binv->apply(u.p, w.p, stop);
    } else {
      A->apply(vcol(j), w.p, stop);
    }
    double *Tcol = T.p + (size_t)j * m;
    orthogonalise(j + 1, stop, Tcol);
    commit(j + 1, j + 1, Tcol, stop, status.p + j + 1, betas.p + j, j > 0 ? tmaxs.p + j - 1 : (double *)nullptr, tmaxs.p + j,
           (m == n && j == n - 1) ? LZ_LAST_OF_FULL_SPACE : LZ_STEP);
  }
  // w holds a vector: (B-)orthogonalise it against the first ncols columns and make it column ncols; status[ncols] = 0 or LZ_NONFINITE
  void new_vector(int ncols) {
    if (gen) B->apply(w.p, u.p, nullptr);
    if (ncols > 0) {
      orthogonalise(ncols, nullptr, nullptr);
    } else {
      hipLaunchKernelGGL(k_lz_update_norm, dim3(g), dim3(NT), lz_lds_bytes(0), s, n, ld, 0, V.p, (const double *)nullptr, w.p,
                         gen ? u.p : (double *)nullptr, (const double *)nullptr, (const double *)nullptr, (double *)nullptr,
                         partn.p, (const int *)nullptr);
      MI_HIP(hipGetLastError());
    }
    commit(0, ncols, nullptr, nullptr, status.p + ncols, beta0.p, nullptr, nullptr, LZ_NEW_VECTOR);
  }

  void run_window(int first) {
    if (!use_graph) {
      for (int j = first; j < m; ++j) step(j);
      return;
    }
    auto it = graphs.find(first);
    if (it == graphs.end()) {
      hipGraphExec_t ex = capture_graph(s, "mi_eigsolve", [&] { for (int j = first; j < m; ++j) step(j); });
      it = graphs.emplace(first, ex).first;
    }
    ++ctx->n_replays;
    MI_HIP(hipGraphLaunch(it->second, s));
  }

  // V[:, :k] = V[:, :mm] * G (and Q likewise); G is mm x k on the host
  void rotate(const std::vector<double> &Gh, int mm, int k, double *dst_or_null) {
    MI_HIP(hipMemcpyAsync(G.p, Gh.data(), sizeof(double) * (size_t)mm * k, hipMemcpyHostToDevice, s));
    for (int pass = 0; pass < (gen && !dst_or_null ? 2 : 1); ++pass) {
      double *P = pass ? Q.p : V.p;
      hipLaunchKernelGGL(k_eig_rotate, dim3(g, k), dim3(NT), sizeof(double) * mm, s, (int)ld, mm, P, G.p, Vtmp.p);
      MI_HIP(hipGetLastError());
      if (dst_or_null)
        MI_HIP(hipMemcpy2DAsync(dst_or_null, sizeof(double) * (size_t)n, Vtmp.p, sizeof(double) * (size_t)ld, sizeof(double) * (size_t)n, k,
                                hipMemcpyDeviceToDevice, s));
      else
        MI_HIP(hipMemcpyAsync(P, Vtmp.p, sizeof(double) * (size_t)ld * k, hipMemcpyDeviceToDevice, s));
    }
    MI_HIP(hipStreamSynchronize(s));  // Gh is the caller's
  }

  // v0_dev: device pointer or nullptr (seeded host vector); vecs_dev: n x nev, device
  int solve(const double *v0_dev, double tol, int64_t maxiter, double *vecs_dev, LanczosResult &out) {
    std::vector<double> hv;
    if (v0_dev) {
      MI_HIP(hipMemcpyAsync(w.p, v0_dev, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, s));
    } else {
      hv.resize(n);
      lz_host_vector(hv, 0);
      MI_HIP(hipMemcpyAsync(w.p, hv.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s));
    }
    new_vector(0);

    std::vector<double> Th((size_t)m * m, 0.0), Td((size_t)m * m), bh(m), theta, Y, rho;
    std::vector<int> sh(m + 1);
    int first = 0, m_eff = m;
    unsigned long long fresh = 0;
    for (;;) {
      run_window(first);
      MI_HIP(hipMemcpyAsync(sh.data(), status.p, sizeof(int) * (m + 1), hipMemcpyDeviceToHost, s));
      MI_HIP(hipMemcpyAsync(bh.data(), betas.p, sizeof(double) * m, hipMemcpyDeviceToHost, s));
      MI_HIP(hipMemcpyAsync(Td.data(), T.p, sizeof(double) * (size_t)m * m, hipMemcpyDeviceToHost, s));
      MI_HIP(hipStreamSynchronize(s));
      int last = m - 1;  // last step that ran
      for (int j = first; j < m; ++j)
        if (sh[j + 1] != LZ_RUN) { last = j; break; }
      if (sh[first] == LZ_NONFINITE)
        return fail(MI_ERR_SINGULAR, "mi_eigsolve: the start vector is zero or not finite (or v0' B v0 is not positive)");
      if (sh[last + 1] == LZ_NONFINITE)
        return fail(MI_ERR_SINGULAR, "mi_eigsolve: step %d met a value that is not finite (beta or T[:, %d])", last, last);
      for (int j = first; j <= last; ++j)
        for (int i = 0; i <= j; ++i) Th[i + (size_t)j * m] = Td[i + (size_t)j * m];
      out.napply += last - first + 1;
      bool finish = false;
      if (sh[last + 1] == LZ_BREAKDOWN) {
        if (last + 1 < nev) {  // continue the basis with a fresh vector; step last+1 computes T[last, last+1] ~ 0 itself
          hv.resize(n);
          lz_host_vector(hv, ++fresh);
          MI_HIP(hipMemcpyAsync(w.p, hv.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s));
          new_vector(last + 1);
          first = last + 1;
          continue;
        }
        m_eff = last + 1;
        finish = true;
      }
      const double beta = bh[last];
      dense::sym_eig_upper(m_eff, Th.data(), m, theta, Y);
      if (which == MI_EIG_LR) {
        std::reverse(theta.begin(), theta.end());
        dense::Mat Yr((size_t)m_eff * m_eff);
        for (int j = 0; j < m_eff; ++j)
          std::copy(Y.begin() + (size_t)(m_eff - 1 - j) * m_eff, Y.begin() + (size_t)(m_eff - j) * m_eff, Yr.begin() + (size_t)j * m_eff);
        Y.swap(Yr);
      }
      rho.resize(m_eff);
      for (int i = 0; i < m_eff; ++i) rho[i] = std::fabs(beta * Y[(m_eff - 1) + (size_t)i * m_eff]);
      int nconv = 0;
      while (nconv < nev && rho[nconv] <= tol) ++nconv;
      out.nconv = nconv;
      if (finish || nconv >= nev || out.nrestart >= maxiter || m_eff == n) break;
      // thick restart
      const int k = std::min(nev + (m - nev) / 2, m - 1);
      std::vector<double> Gh(Y.begin(), Y.begin() + (size_t)m * k);
      rotate(Gh, m, k, nullptr);
      MI_HIP(hipMemcpyAsync(vcol(k), vcol(m), sizeof(double) * (size_t)ld, hipMemcpyDeviceToDevice, s));
      if (gen) MI_HIP(hipMemcpyAsync(qcol(k), qcol(m), sizeof(double) * (size_t)ld, hipMemcpyDeviceToDevice, s));
      std::fill(Th.begin(), Th.end(), 0.0);
      double tmax = 0.0;
      for (int i = 0; i < k; ++i) { Th[i + (size_t)i * m] = theta[i]; tmax = std::max(tmax, std::fabs(theta[i])); }
      const int zero = LZ_RUN;
      MI_HIP(hipMemcpyAsync(tmaxs.p + k - 1, &tmax, sizeof(double), hipMemcpyHostToDevice, s));
      MI_HIP(hipMemcpyAsync(status.p + k, &zero, sizeof(int), hipMemcpyHostToDevice, s));
      MI_HIP(hipStreamSynchronize(s));  // tmax and zero are on this stack frame
      first = k;
      ++out.nrestart;
    }
    out.vals.assign(theta.begin(), theta.begin() + nev);
    out.resid.assign(rho.begin(), rho.begin() + nev);
    std::vector<double> Gh(Y.begin(), Y.begin() + (size_t)m_eff * nev);
    rotate(Gh, m_eff, nev, vecs_dev);
    return MI_OK;
  }
};

}  // namespace mi
