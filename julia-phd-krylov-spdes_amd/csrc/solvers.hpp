// cg / pcg / defcg / defpcg with the whole loop on the device (RecyclingKrylovSolvers/cg.jl, defcg.jl).
//
// One iteration is a fixed sequence of kernel launches whose scalars (alpha, beta, r'r, r'z, it,
// the stop flag) live in HBM (`SolverState`), so the host never reads a scalar inside the loop.
// Iterations are captured into hipGraphs and replayed; launches that follow the iteration at which
// the stop rule fired return immediately (`done`), so the iterates, `it` and `res_norm` are exactly
// those of the reference's `while (it < maxit) && (res_norm[it] > tol)` whatever the replay sizes.
//
// Replay policy: the first replay holds the set-up (r = b - A x, z = M \ r, p = z, it = 1) plus as
// many iterations as the previous solve with the same (A, M) needed, so a repeated or similar solve
// (Example07's realization loop) is ONE graph launch and ONE host wait; result copies are enqueued
// speculatively behind it. If the stop flag is not up, `chunk`-sized replays follow, the host
// looking at the flag of the PREVIOUS replay (one replay of run-ahead).
#pragma once
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <tuple>

#include "eig_kernels.hpp"
#include "operators.hpp"

namespace mi {

constexpr int64_t RES_STAGE = 8192;
constexpr int CF_VEC_GRID = 256;  // workgroups of the vector half of the 2-launch sparse pcg (8 XCDs x 32) = partials per dot (<= NT)

struct GraphKey {
  const Operator *A, *M;
  int nvec, chunk;  // chunk > 0: that many iterations; chunk < 0: set-up + (-chunk) iterations
  int tag = 0;      // whatever else decides the launches of a graph, set by Krylov::graph (0 in the keys of `predicted` / `zero_x0`)
  bool operator<(const GraphKey &o) const {
    return std::tie(A, M, nvec, chunk, tag) < std::tie(o.A, o.M, o.nvec, o.chunk, o.tag);
  }
};

struct SolverWorkspace {
  int64_t n = 0;
  int g = 1;  // workgroups of the multi-workgroup vector kernels = number of partials per dot
  // One slab for the state, the partials and the six work vectors: the latency-bound loop kernels
  // then touch a handful of pages instead of one per allocation.
  DevBuf<char> slab;
  SolverState *st = nullptr;
  double *part_pAp = nullptr, *part_rr = nullptr, *part_rz = nullptr, *part_bb = nullptr;
  double *r = nullptr, *z = nullptr, *p = nullptr, *Ap = nullptr, *x = nullptr, *b = nullptr;
  DevBuf<double> res_norm;
  // deflation
  DevBuf<double> W, AW, LU, mu, part_mu, gram;
  DevBuf<double> fold_mu, fold_wm;  // folded Def-PCG: per-tile partials of WtA*z, (W*mu) in local order
  DevBuf<double> fold_wloc;         //                  W in the local order of the blocks (nvec x nloc), gathered per solve
  DevBuf<long long> fold_dbg;       // MI355_FOLD_DEBUG=1: 64 launches x 8 stamps of one workgroup of the folded launches
  DevBuf<double> cf_pz, cf_rr, cf_rz;  // 2-launch sparse pcg: two buffers of interleaved (p, z) pairs, per-block partials
  DevBuf<int> piv;
  int nvec_cap = 0;
  // eigCG family (eig_solvers.hpp): search space V (n x spdim), A*V (eigpcg), rotation target, tvec, VtAV, ...
  DevBuf<double> eV, eAV, eVtmp, etvec, eT, eG, epart, eLUw, emu2;
  DevBuf<int> epivw;
  DevBuf<EigState> ees;
  int e_spdim = 0, e_nvec = 0;
  bool e_av = false;
  PinnedFlags *flags = nullptr;    // 2 slots, pinned
  SolveArgs *args = nullptr;       // pinned: per-call arguments of a whole-solve graph (k_solve_begin_g)
  DevBuf<SolveArgs> args_dev;      // its device copy for k_solve_end_g, + the exit kernel's workgroup counter
  DevBuf<unsigned> end_count;
  unsigned long long seq = 0;
  // MI355_SOLVE_STATS=1: every 64 whole-graph solves, the average device span (entry kernel's start .. hand-over) and the
  // average host period between hand-overs go to stderr (period - span = host turnaround + launch latency)
  bool stats_on = env_int("MI355_SOLVE_STATS", 0) != 0;
  long long stat_span = 0;
  int stat_n = 0;
  std::chrono::steady_clock::time_point stat_t0;
  void stat(long long span_ticks) {
    const auto now = std::chrono::steady_clock::now();
    if (stat_n == 0) stat_t0 = now;
    else stat_span += span_ticks;
    if (++stat_n == 65) {
      const double period = std::chrono::duration<double, std::micro>(now - stat_t0).count() / 64.0;
      std::fprintf(stderr, "[mi355 solve stats] n=%lld: device span %.2f us, host period %.2f us\n", (long long)n, stat_span * 0.01 / 64.0, period);
      stat_n = 0; stat_span = 0;
    }
  }
  double *res_stage = nullptr;     // pinned landing zone for short residual histories
  hipEvent_t ev[2] = {nullptr, nullptr};
  std::map<GraphKey, hipGraphExec_t> graphs;
  std::map<GraphKey, int> predicted;  // loop iterations the last solve with this (A, M, nvec) took
  std::map<GraphKey, bool> zero_x0;   // ... and whether its initial guess was identically zero (whole-solve graphs)

  explicit SolverWorkspace(int64_t n_) : n(n_), g(vec_grid(n_)) {
    auto pad = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t vec = pad(sizeof(double) * ((size_t)n + 2)), part = pad(sizeof(double) * MAX_PARTS);
    const size_t total = pad(sizeof(SolverState)) + 4 * part + 6 * vec;
    slab.alloc(total);
    memset_sync(slab.p, 0, total);
    char *q = slab.p;
    st = (SolverState *)q; q += pad(sizeof(SolverState));
    part_pAp = (double *)q; q += part; part_rr = (double *)q; q += part;
    part_rz = (double *)q; q += part; part_bb = (double *)q; q += part;
    r = (double *)q; q += vec; z = (double *)q; q += vec; p = (double *)q; q += vec;
    Ap = (double *)q; q += vec; x = (double *)q; q += vec; b = (double *)q; q += vec;
    MI_HIP(hipHostMalloc((void **)&flags, 2 * sizeof(PinnedFlags)));
    std::memset(flags, 0, 2 * sizeof(PinnedFlags));
    MI_HIP(hipHostMalloc((void **)&args, sizeof(SolveArgs)));
    if (env_int("MI355_FOLD_DEBUG", 0)) { fold_dbg.alloc(512); memset_sync(fold_dbg.p, 0, 512 * sizeof(long long)); }
    args_dev.alloc(1); end_count.alloc(1);
    memset_sync(end_count.p, 0, sizeof(unsigned));
    MI_HIP(hipHostMalloc((void **)&res_stage, RES_STAGE * sizeof(double)));
    for (auto &e : ev) MI_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  ~SolverWorkspace() {
    drop_graphs();
    if (flags) (void)hipHostFree(flags);
    if (args) (void)hipHostFree(args);
    if (res_stage) (void)hipHostFree(res_stage);
    for (auto &e : ev) if (e) (void)hipEventDestroy(e);
  }
  void drop_graphs() {
    for (auto &kv : graphs) (void)hipGraphExecDestroy(kv.second);
    graphs.clear();
  }
  // Every graph, and every prediction, of a solve whose A or M is `op` or applies `op` (Operator::uses): a graph of a
  // combined M holds the launch arguments of its children. The operators of the keys are alive: mi_op_destroy calls
  // this before it deletes one, and refuses an operator that another one borrows.
  void drop_graphs_of(const Operator *op) {
    auto of_op = [op](const GraphKey &k) { return (k.A && k.A->uses(op)) || (k.M && k.M->uses(op)); };
    for (auto &kv : graphs) if (of_op(kv.first)) (void)hipGraphExecDestroy(kv.second);
    auto erase_of = [&](auto &map) { for (auto it = map.begin(); it != map.end();) it = of_op(it->first) ? map.erase(it) : std::next(it); };
    erase_of(graphs); erase_of(predicted); erase_of(zero_x0);
  }
  void ensure_deflation(int nvec) {
    if (nvec <= nvec_cap) return;
    drop_graphs();  // buffers move
    W.alloc((size_t)n * nvec); AW.alloc((size_t)n * nvec);
    LU.alloc((size_t)nvec * nvec); gram.alloc((size_t)nvec * nvec);
    mu.alloc(nvec); piv.alloc(nvec); part_mu.alloc((size_t)nvec * MAX_PARTS);
    nvec_cap = nvec;
  }
  void ensure_eig(int spdim, int nvec, bool need_av) {
    if (spdim <= e_spdim && nvec <= e_nvec && (!need_av || e_av)) return;
    drop_graphs();
    spdim = std::max(spdim, e_spdim); nvec = std::max(nvec, e_nvec); need_av = need_av || e_av;
    eV.alloc((size_t)n * spdim); eVtmp.alloc((size_t)n * 2 * nvec); etvec.alloc((size_t)n);
    if (need_av) eAV.alloc((size_t)n * spdim);
    eT.alloc((size_t)spdim * spdim); eG.alloc((size_t)spdim * 2 * nvec); epart.alloc((size_t)2 * nvec * MAX_PARTS);
    eLUw.alloc((size_t)nvec * nvec); emu2.alloc(nvec); epivw.alloc(nvec); ees.alloc(1);
    e_spdim = spdim; e_nvec = nvec; e_av = need_av;
  }
};

inline SolverWorkspace &workspace(mi_ctx_s *ctx, int64_t n) {
  auto &slot = ctx->workspaces[n];
  if (!slot) slot.reset(new SolverWorkspace(n));
  return *slot;
}

// LAPACK getrf (unblocked, partial pivoting) on a column-major copy. Returns 0 or k+1 for U[k,k]==0. A pivot that is NaN or
// Inf is no zero pivot: getrf reports info = 0 and `WtAW \ mu` returns NaN, which ends the solve at it = 1 (res_norm[1] = NaN).
inline int host_lu(int n, std::vector<double> &a, std::vector<int> &piv) {
  piv.resize(n);
  for (int k = 0; k < n; ++k) {
    int p = k;
    double mx = std::fabs(a[k + (size_t)k * n]);
    for (int i = k + 1; i < n; ++i) {
      const double v = std::fabs(a[i + (size_t)k * n]);
      if (v > mx) { mx = v; p = i; }
    }
    piv[k] = p;
    if (a[p + (size_t)k * n] == 0.0) return k + 1;
    if (p != k)
      for (int j = 0; j < n; ++j) std::swap(a[k + (size_t)j * n], a[p + (size_t)j * n]);
    const double piv_inv = 1.0 / a[k + (size_t)k * n];
    for (int i = k + 1; i < n; ++i) a[i + (size_t)k * n] *= piv_inv;
    for (int j = k + 1; j < n; ++j) {
      const double akj = a[k + (size_t)j * n];
      for (int i = k + 1; i < n; ++i) a[i + (size_t)j * n] -= a[i + (size_t)k * n] * akj;
    }
  }
  return 0;
}

// The form of the loop: which kernels make one iteration. Exclusive, chosen once per solver by Krylov::select_form (table: DESIGN §3).
// GENERIC: multi-workgroup vector kernels around plain applies. FUSED: n <= FUSED_MAX_N, single-workgroup vector kernels over slot views. FOLD:
// pcg, both operators dense on the same maps, the vector work inside the two GEMVs; FOLD_BIG: the same beyond FUSED_MAX_N. CSRFOLD: cg / diagonal pcg on a CSR matrix.
enum class Loop { GENERIC, FUSED, FOLD, FOLD_BIG, CSRFOLD };

struct Krylov {
  mi_ctx_s *ctx;
  Operator *A, *M;  // M == nullptr: unpreconditioned (z is r)
  const int pre;    // M != nullptr
  SolverWorkspace &ws;
  int nvec;
  int n, g;
  hipStream_t s;
  Loop form = Loop::GENERIC;
  CsrDev *Ac = nullptr;                        // CSRFOLD: A
  DenseBlockOp *Ad = nullptr, *Md = nullptr;   // FOLD, FOLD_BIG: A and M
  bool two_launch() const { return form == Loop::FOLD || form == Loop::FOLD_BIG || form == Loop::CSRFOLD; }  // the host reads it_nxt
  bool folded() const { return form == Loop::FOLD || form == Loop::FOLD_BIG; }
  bool single_wg() const { return form == Loop::FUSED || form == Loop::FOLD; }  // the single-workgroup kernels leave z, Ap as slot views
  int capture_whole = 0;  // while a whole-solve graph is being captured: 1 general entry, 2 entry for x0 == 0 (folded loop)
  // eigCG family: recording kernels after every iteration (eig_solvers.hpp fills this in)
  struct EigHook {
    int tag = 0, spdim = 0;
    bool has_tvec = false;   // eigcg / eigpcg keep tvec and the coupling column
    bool project_r = false;  // eigdefpcg: r .-= W * (WtW \ (W' * r)) before rTr (defcg.jl:411)
  } eig;
  std::vector<double> gram_host;  // WtAW as computed (before LU), kept for VtAV[1:nvec,1:nvec] (defcg.jl:158 / 391)

  // generic: GENERIC whatever the size. recording: the eigCG family reads z and Ap after every iteration, so no two-launch form.
  Krylov(mi_ctx_s *c, Operator *A_, Operator *M_, int nvec_, bool generic = false, bool recording = false)
      : ctx(c), A(A_), M(M_), pre(M_ != nullptr), ws(workspace(c, A_->n)), nvec(nvec_), n((int)A_->n), g(ws.g), s(c->stream) {
    select_form(generic, recording);
  }
  void select_form(bool generic, bool recording) {
    const bool fused = !generic && A->n <= FUSED_MAX_N && !env_int("MI355_NO_FUSED", 0);
    form = fused ? Loop::FUSED : Loop::GENERIC;
    // (the folded launches themselves are multi-workgroup: beyond FUSED_MAX_N only the start-up differs — the
    // reference's own partitions, 80-500 subdomains, have n_Γ of 10-40 k; undeflated solves only there)
    const bool big_fold = !fused && !generic && nvec == 0 && !env_int("MI355_NO_FUSED", 0) && !env_int("MI355_NO_BIG_FOLD", 0);
    if ((fused || big_fold) && !recording && M && nvec <= 64 && !env_int("MI355_NO_FOLD", 0) && !(nvec > 0 && env_int("MI355_NO_FOLD_DEFL", 0))) {
      Ad = A->as_dense(); Md = M->as_dense();
      // multi-GPU: S may be sharded (built on the maps of all subdomains, inactive tiles for the other ranks' blocks)
      // while the Neumann-Neumann blocks are replicated: the S launch is then followed by one all-reduce
      // ... or sharded as well (both on the maps of all subdomains): then the ΠS launch is followed by an exchange too
      const bool fold = Ad && Md && (!Ad->reduce_over_ranks || (Ad->full_maps && nvec == 0)) &&
             (!Md->reduce_over_ranks || (Md->full_maps && Md->fold_p1_off && nvec == 0 && !env_int("MI355_NO_FOLD_SHARDED_NN", 0))) &&
             !Ad->scale && Md->scale && Ad->same_maps(*Md) && Ad->ntiles > 0 && Ad->max_ld <= GEMV_PANEL && Md->max_ld <= GEMV_PANEL &&
             Ad->maps.slot_width <= 4 &&
             // fp32-stored ΠS: folded when it is a local operator (one GPU, or replicated beside a sharded S); a SHARDED
             // fp32 ΠS takes the unfolded loop (plain applies + all-reduce) — its launch has no peer-exchange form
             !(Md->f32() && Md->reduce_over_ranks) &&
             (Ad->max_ld + 64 * Ad->waves - 1) / (64 * Ad->waves) <= 8 && (Md->max_ld + 64 * Md->waves - 1) / (64 * Md->waves) <= 8;
      if (fold) form = fused ? Loop::FOLD : Loop::FOLD_BIG;
    }
    const double *dv = nullptr;
    if (form == Loop::GENERIC && !recording && nvec == 0 && A->as_csr() && A->as_csr()->nblocks > 0 && (!M || M->diag_kind(&dv) != 0) &&
        !env_int("MI355_NO_CSRFOLD", 0)) { Ac = A->as_csr(); form = Loop::CSRFOLD; }
  }
  // peer exchange with the waits inside the launches: every sharded operator of the loop stores into the arenas itself
  bool inwait() const {
    // (an fp32-stored ΠS launch cannot wait inside itself: the one-wave wait kernel runs behind the S launch instead)
    return folded() && !Md->f32() && ctx->peer_inwait && ctx->use_peer() && (Ad->reduce_over_ranks || Md->reduce_over_ranks) &&
           (!Ad->reduce_over_ranks || (Ad->xt_on() && Ad->xt_direct)) && (!Md->reduce_over_ranks || (Md->xt_on() && Md->xt_direct));
  }
  PcgFold fold_args(int phase) const {
    PcgFold f{};
    const size_t nl = (size_t)Ad->maps.nloc;
    f.st = ws.st; f.W = Ad->maps.slot_width; f.res_norm = ws.res_norm.p; f.x = ws.x; f.r_gamma = ws.r;
    f.r_cur = Ad->fold_vec.p; f.r_nxt = f.r_cur + nl; f.p_cur = f.r_nxt + nl; f.p_nxt = f.p_cur + nl;
    f.tgt = Ad->maps.tgt.p; f.peer = Ad->maps.peer.p; f.jrank = Ad->maps.jrank.p;
    // partial-dot arrays of the OTHER operator's launch (tilings may differ); a sharded S writes one product per row
    f.nvec = nvec; f.n_gamma = n;
    if (nvec > 0) { f.AW = ws.AW.p; f.part_mu = ws.fold_mu.p; f.wm_loc = ws.fold_wm.p; }
    if (capture_whole && phase == 0) { f.exit_args = ws.args_dev.p; f.exit_flags = &ws.flags[0]; }
    if (ws.fold_dbg.p) { f.dbg = ws.fold_dbg.p; f.dbg_wg = env_int("MI355_FOLD_DEBUG_WG", 0); }
    // a sharded launch's outputs are exchanged over the ranks before the other launch reads them (reduced copy of the pack;
    // with the peer exchange a double-buffered table whose parity the reading launch takes from the exchange counter)
    const bool redA = Ad->reduce_over_ranks, redM = Md->reduce_over_ranks;
    f.n_in = phase ? Ad->part_total : Md->part_total;
    if (phase) {  // ΠS launch: reads S contributions + partial p'Ap, writes ΠS contributions + partial r'r, r'z
      f.con_in = Ad->fold_con(redA);
      f.part_in0 = Ad->fold_part0(redA); f.part_in1 = nullptr;
      Md->fold_outputs(f);
      if (redA && Ad->xt_on()) { f.in_epoch = &ctx->peer->st->epoch; f.in_stride = (long long)Ad->xt_copy; }
    } else {      // S launch: reads ΠS contributions + partial r'r, r'z, writes S contributions + partial p'Ap
      f.con_in = Md->fold_con(redM);
      f.part_in0 = Md->fold_part0(redM); f.part_in1 = Md->fold_part1p(redM);
      Ad->fold_outputs(f);
      if (redM && Md->xt_on()) { f.in_epoch = &ctx->peer->st->epoch; f.in_stride = (long long)Md->xt_copy; }
    }
    if (inwait()) { f.x_inwait = 1; f.xst = ctx->peer->st; f.xpw = ctx->peer->peers_dev; }
    // A sharded operator's tiling is its rank's own (operators.hpp): its launch sums the partials it reads in an order
    // that does not depend on it. (A replicated operator has one tiling on all ranks.)
    f.canon = (phase ? Md : Ad)->reduce_over_ranks ? 1 : 0;
    return f;
  }

  const int *done() const { return &ws.st->done; }

  void dot_partial(const double *x, const double *y, double *part, const int *dn) {
    hipLaunchKernelGGL(k_dot_partial, dim3(g), dim3(NT), 0, s, n, x, y, part, dn);
    MI_HIP(hipGetLastError());
  }
  // mu = WtAW \ (V' v), V = AW (loop) or W (set-up)
  void project(const double *V, const double *v, const int *dn) { project(V, v, dn, ws.LU.p, ws.piv.p, ws.mu.p); }
  void project(const double *V, const double *v, const int *dn, const double *LU, const int *piv, double *mu) {
    hipLaunchKernelGGL(k_multi_dot_partial, dim3(g, nvec), dim3(NT), 0, s, n, V, v, ws.part_mu.p, dn);
    hipLaunchKernelGGL(k_lu_solve, dim3(1), dim3(64), sizeof(double) * (nvec <= 64 ? nvec + nvec * nvec + nvec / 2 + 1 : nvec), s, nvec, LU, piv,
                       ws.part_mu.p, g, mu, dn);
    MI_HIP(hipGetLastError());
  }
  // z (what p is updated with) and Ap of the current iteration as the loop in use leaves them: slot views in the fused
  // loop, plain vectors in the multi-workgroup one
  AsmView z_view() const {
    if (!M) return AsmView{ws.r, 0};
    return single_wg() && nvec == 0 ? M->view_of(ws.z) : AsmView{ws.z, 0};
  }
  AsmView Ap_view() const { return single_wg() ? A->view_of(ws.Ap) : AsmView{ws.Ap, 0}; }
  // Lanczos bookkeeping of the eigCG family for the iteration just enqueued
  void eig_record() {
    double *tv = eig.has_tvec ? ws.etvec.p : nullptr;
    hipLaunchKernelGGL(k_eig_vec, dim3(g), dim3(NT), 0, s, n, ws.st, ws.ees.p, pre, eig.spdim, z_view(), Ap_view(), ws.eV.p, tv);
    if (eig.has_tvec)
      hipLaunchKernelGGL(k_eig_coupling, dim3(g, 2 * ws.e_nvec), dim3(NT), 0, s, n, ws.st, ws.ees.p, ws.eV.p, ws.etvec.p,
                         ws.epart.p);
    hipLaunchKernelGGL(k_eig_state, dim3(1), dim3(64), 0, s, ws.st, ws.ees.p, ws.eT.p, eig.spdim, ws.epart.p, g,
                       (int)eig.has_tvec);
    MI_HIP(hipGetLastError());
  }

  // launch(std::integral_constant<int, EPT>): the single-workgroup kernels are instantiated per elements per thread, 1, 2, 4 or 8
  template <class F>
  void with_ept(F launch) const {
    if (n <= NTF) launch(std::integral_constant<int, 1>{});
    else if (n <= 2 * NTF) launch(std::integral_constant<int, 2>{});
    else if (n <= 4 * NTF) launch(std::integral_constant<int, 4>{});
    else launch(std::integral_constant<int, 8>{});
  }
  // One loop iteration (cg.jl:35-47 / 92-106; defcg.jl:68-80 / 291-305), enqueued on the stream.
  void iteration() {
    switch (form) {
      case Loop::FOLD: case Loop::FOLD_BIG: return iter_fold();
      case Loop::FUSED: return iter_fused();
      case Loop::CSRFOLD: return iter_csrfold();
      case Loop::GENERIC: return iter_generic();
    }
  }
  // 2 launches per iteration: (alpha, x, r, z, r'z, r'r) in the ΠS GEMV; (stop rule, beta, p, Ap, p'Ap) in the S GEMV
  void iter_fold() {
    const int *dn = done();
    Md->gemv_pcg(1, fold_args(1));
    if (Md->reduce_over_ranks) Md->reduce_fold(dn, inwait());  // ΠS contributions + partial r'r, r'z: union over the ranks
    if (nvec > 0) {  // mu = WtAW \ (WtA * z); W*mu in local order for the S launch (defcg.jl:301-303)
      hipLaunchKernelGGL(k_defl_mu, dim3((Ad->maps.nloc + 1023) / 1024), dim3(1024), 0, s, ws.st, nvec, Md->ntiles, ws.fold_mu.p,
                         ws.LU.p, ws.piv.p, Ad->maps.nloc, Ad->maps.gidx.p, ws.W.p, (long long)n, ws.fold_wm.p, ws.mu.p, ws.fold_wloc.p);
      MI_HIP(hipGetLastError());
    }
    Ad->gemv_pcg(0, fold_args(0));
    if (Ad->reduce_over_ranks) Ad->reduce_fold(dn, inwait());  // S contributions + partial p'Ap: union over the ranks
  }
  // small Γ systems: 4 launches per iteration (GEMV, fused, GEMV, fused)
  void iter_fused() {
    const int *dn = done();
    const double *Wp = nvec > 0 ? ws.W.p : nullptr, *mup = nvec > 0 ? ws.mu.p : nullptr;
    const AsmView vAp = A->apply_view(ws.p, ws.Ap, dn);             // mul!(Ap, A, p), Γ-sum deferred
    if (!pre && nvec == 0) {                                        // cg: 2 launches per iteration
      with_ept([&](auto E) { hipLaunchKernelGGL((k_fused_cg<E()>), dim3(1), dim3(NTF), 0, s, n, ws.st, vAp, ws.p, ws.x, ws.r, ws.res_norm.p); });
      if (eig.tag) eig_record();
      MI_HIP(hipGetLastError());
      return;
    }
    // alpha; x += alpha p; r -= alpha Ap; r'r
    with_ept([&](auto E) { hipLaunchKernelGGL((k_fused_xr<E()>), dim3(1), dim3(NTF), 0, s, n, ws.st, vAp, ws.p, ws.x, ws.r, pre); });
    AsmView vz{ws.r, 0};
    if (pre) vz = M->apply_view(ws.r, ws.z, dn);                    // z .= M \ r, Γ-sum deferred
    const bool wave_lu = nvec > 0 && nvec <= 64;                    // mu solved inside k_fused_p by one wave
    if (wave_lu) {  // WtA * z
      with_ept([&](auto E) { hipLaunchKernelGGL((k_multi_dot_view<E()>), dim3(nvec), dim3(NTF), 0, s, n, ws.AW.p, vz, ws.part_mu.p, dn); });
    } else if (nvec > 0) {
      if (vz.width) {  // materialise z for the generic projection kernels
        hipLaunchKernelGGL(k_assemble_slots, dim3(vec_grid(n)), dim3(NT), 0, s, n, vz.width, vz.src, ws.z, dn);
        vz = AsmView{ws.z, 0};
      }
      project(ws.AW.p, vz.src, dn);                                 // mu .= WtAW \ (WtA * z)
    }
    const double *lup = wave_lu ? ws.LU.p : nullptr; const int *pivp = wave_lu ? ws.piv.p : nullptr;
    // beta; [mu;] p; it += 1; res_norm[it]; stop rule
    with_ept([&](auto E) { hipLaunchKernelGGL((k_fused_p<E()>), dim3(1), dim3(NTF), 0, s, n, ws.st, vz, ws.r, ws.p, Wp, mup, nvec, ws.res_norm.p, pre, lup, pivp, ws.part_mu.p); });
    if (eig.tag) eig_record();
    MI_HIP(hipGetLastError());
  }
  // sparse A, diagonal or no M: 2 launches per iteration (kernels.hpp, "pcg on a sparse matrix in 2 launches")
  void iter_csrfold() {
    const double *dinv = nullptr;
    const int diag = pre ? M->diag_kind(&dinv) : 0;
    const int grid = ((Ac->nblocks + 7) / 8) * 8;
    double *pz0 = ws.cf_pz.p, *pz1 = pz0 + 2 * (size_t)n;
    CsrOp *co = static_cast<CsrOp *>(A);
    hipLaunchKernelGGL(k_spmv_pcg, dim3(grid), dim3(NT), 0, s, Ac->nblocks, pre, Ac->blk.p, ws.st, ws.cf_rr.p, ws.cf_rz.p, CF_VEC_GRID,
                       Ac->rowptr.p, Ac->col.p, Ac->val.p, pz0, pz1, ws.Ap, co->dot_part.p, ws.res_norm.p);
    hipLaunchKernelGGL(k_update_xr_blk, dim3(CF_VEC_GRID), dim3(NT), 0, s, Ac->xcd_row.p, ws.st, co->dot_part.p, Ac->nblocks, pz0,
                       pz1, ws.Ap, ws.x, ws.r, dinv, diag, pre, ws.cf_rr.p, ws.cf_rz.p);
    MI_HIP(hipGetLastError());
  }
  // large systems (full A): SpMV with the p'Ap partials in its epilogue; r-update with a diagonal M folded in
  void iter_generic() {
    const int *dn = done();
    const double *Wp = nvec > 0 ? ws.W.p : nullptr, *mup = nvec > 0 ? ws.mu.p : nullptr;
    const double *part = ws.part_pAp;
    int npart = g;
    if (!A->apply_dot(ws.p, ws.Ap, ws.p, &part, &npart, dn)) {       // mul!(Ap, A, p); d = dot(p, Ap)
      A->apply(ws.p, ws.Ap, dn);
      dot_partial(ws.p, ws.Ap, ws.part_pAp, dn);
      part = ws.part_pAp; npart = g;
    }
    const double *dinv = nullptr;
    const int diag = pre && !eig.project_r ? M->diag_kind(&dinv) : 0;
    hipLaunchKernelGGL(k_update_xr, dim3(g), dim3(NT), 0, s, n, ws.st, part, npart, ws.p, ws.Ap, ws.x, ws.r,
                       ws.part_rr, pre, diag, dinv, ws.z, ws.part_rz);  // alpha; x += alpha p; r -= alpha Ap; r'r [; z; r'z]
    if (eig.project_r) {                                                // r .-= W * (WtW \ (W' * r)); rTr = dot(r, r)
      project(ws.W.p, ws.r, dn, ws.eLUw.p, ws.epivw.p, ws.emu2.p);
      hipLaunchKernelGGL(k_project_r, dim3(g), dim3(NT), 0, s, n, ws.r, ws.W.p, ws.emu2.p, nvec, ws.part_rr, dn);
    }
    const double *zz = ws.r;
    if (pre) {
      if (!diag) {
        M->apply(ws.r, ws.z, dn);                                     // z .= M \ r
        dot_partial(ws.r, ws.z, ws.part_rz, dn);                      // rTz = dot(r, z)
      }
      zz = ws.z;
    }
    if (nvec > 0) project(ws.AW.p, zz, dn);                           // mu .= WtAW \ (WtA * z)
    hipLaunchKernelGGL(k_update_p, dim3(g), dim3(NT), 0, s, n, ws.st, ws.part_rr, ws.part_rz, g, zz, ws.p, Wp, mup, nvec,
                       ws.res_norm.p, pre);                           // beta; p; it += 1; res_norm[it]; stop rule
    if (eig.tag) eig_record();
    MI_HIP(hipGetLastError());
  }

  // r = b - A x; z = M \ r; p = z [- W mu]; it = 1; res_norm[1]; tol (cg.jl:26-33 / 81-89; defcg.jl:56-66 / 277-288).
  // eps / maxit / res_cap are read from the state block (uploaded by solve()), so this is graph-replayable.
  void setup_tail() {
    switch (form) {
      case Loop::FOLD_BIG: return start_fold_big();
      case Loop::FOLD: return start_fold();
      case Loop::FUSED: return nvec == 0 ? start_fused() : start_generic();  // (the deflated set-up has multi-workgroup kernels only)
      case Loop::CSRFOLD: return start_csrfold();
      case Loop::GENERIC: return start_generic();
    }
  }
  struct Hint {  // `A*x0` may skip streaming A when the device flag says x0 == 0 (k_solve_begin)
    Operator *op;
    Hint(Operator *o, const int *flag) : op(o) { op->zero_hint = flag; }
    ~Hint() { op->zero_hint = nullptr; }
  };
  void start_residual() {  // r = b - A x and the partials of r'r, b'b with the multi-workgroup kernels
    { Hint h(A, nvec == 0 ? &ws.st->x0_zero : nullptr); A->apply(ws.x, ws.Ap, nullptr); }  // deflated: x0 was updated by W*mu
    hipLaunchKernelGGL(k_residual, dim3(g), dim3(NT), 0, s, n, ws.b, ws.Ap, ws.r, ws.part_rr, ws.part_bb);
  }
  // n_Γ > FUSED_MAX_N (undeflated): multi-workgroup residual, then the scalars of the folded loop
  void start_fold_big() {
    start_residual();
    hipLaunchKernelGGL(k_fold_start, dim3(1), dim3(NT), 0, s, ws.st, ws.part_rr, ws.part_bb, g);
    MI_HIP(hipGetLastError());
    if (inwait()) ctx->peer->begin_inwait(s);
  }
  void start_fold() {
    AsmView vAp;
    { Hint h(A, nvec == 0 ? &ws.st->x0_zero : nullptr); vAp = A->apply_view(ws.x, ws.Ap, nullptr); }  // deflated: x0 was updated by W*mu
    with_ept([&](auto E) { hipLaunchKernelGGL((k_fused_residual<E(), true>), dim3(1), dim3(NTF), 0, s, n, ws.st, vAp, ws.b, ws.r); });
    MI_HIP(hipGetLastError());
    if (inwait()) ctx->peer->begin_inwait(s);
  }
  void start_fused() {
    AsmView vAp;
    { Hint h(A, &ws.st->x0_zero); vAp = A->apply_view(ws.x, ws.Ap, nullptr); }
    with_ept([&](auto E) { hipLaunchKernelGGL((k_fused_residual<E(), false>), dim3(1), dim3(NTF), 0, s, n, ws.st, vAp, ws.b, ws.r); });
    const AsmView vz = pre ? M->apply_view(ws.r, ws.z, nullptr) : AsmView{ws.r, 0};
    with_ept([&](auto E) { hipLaunchKernelGGL((k_fused_start<E()>), dim3(1), dim3(NTF), 0, s, n, ws.st, vz, ws.r, ws.p, ws.res_norm.p, pre); });
    MI_HIP(hipGetLastError());
  }
  void start_csrfold() {
    start_residual();
    const double *dinv = nullptr;
    const int diag = pre ? M->diag_kind(&dinv) : 0;
    if (diag == 2) {
      M->apply(ws.r, ws.z, nullptr);
      dot_partial(ws.r, ws.z, ws.part_rz, nullptr);
    }
    hipLaunchKernelGGL(k_csrfold_start, dim3(g), dim3(NT), 0, s, n, CF_VEC_GRID, ws.st, ws.part_rr, ws.part_bb,
                       diag == 2 ? ws.part_rz : (const double *)nullptr, g, diag == 2 ? ws.z : ws.r, ws.cf_pz.p, ws.cf_rr.p,
                       ws.cf_rz.p);
    MI_HIP(hipGetLastError());
  }
  void start_generic() {
    start_residual();
    const double *zz = ws.r;
    if (pre) {
      M->apply(ws.r, ws.z, nullptr);
      dot_partial(ws.r, ws.z, ws.part_rz, nullptr);
      zz = ws.z;
    }
    hipLaunchKernelGGL(k_init_state, dim3(1), dim3(NT), 0, s, ws.st, ws.part_rr, ws.part_bb,
                       pre ? ws.part_rz : (const double *)nullptr, g, ws.res_norm.p);
    if (nvec > 0) project(ws.AW.p, zz, nullptr);
    hipLaunchKernelGGL(k_init_p, dim3(g), dim3(NT), 0, s, n, zz, ws.p, nvec > 0 ? ws.W.p : (const double *)nullptr,
                       nvec > 0 ? ws.mu.p : (const double *)nullptr, nvec);
    MI_HIP(hipGetLastError());
  }

  // chunk > 0: `chunk` iterations; chunk < 0: set-up tail + (-chunk) iterations; whole: the entry kernel in front of
  // and the exit kernel behind them (arguments through ws.args), so that a solve is ONE replay.
  // (Splitting a whole-solve graph into a short head and the rest, so that the GPU starts while the host still enqueues,
  // was measured: 432 vs 427 us per solve — one replay is cheaper than two.)
  hipGraphExec_t graph(int chunk, int whole = 0) {
    // tag: the loop form (0 ... 4), the whole-solve entry (0: none, 1: general, 2: for x0 == 0), the eigCG family's recording (eig.tag)
    GraphKey key{A, M, nvec, chunk, (int)form + 8 * (whole + 4 * eig.tag)};
    auto it = ws.graphs.find(key);
    if (it != ws.graphs.end()) return it->second;
    hipGraphExec_t ex = nullptr;
    try {
      ex = capture_graph(s, "", [&] {
        capture_whole = whole;
        if (whole == 2) {   // folded loop, x0 == 0: one entry launch
          with_ept([&](auto E) { hipLaunchKernelGGL((k_entry_zero<E()>), dim3(1), dim3(NTF), 0, s, n, ws.args, ws.b, ws.x, ws.r, ws.st, ws.args_dev.p, &ws.flags[0]); });
          MI_HIP(hipGetLastError());
        } else {
          if (whole) {
            hipLaunchKernelGGL(k_solve_begin_g, dim3(g), dim3(NT), 0, s, n, ws.args, ws.b, ws.x, ws.st, ws.args_dev.p, &ws.flags[0]);
            MI_HIP(hipGetLastError());
          }
          if (chunk < 0) setup_tail();
        }
        for (int k = 0; k < std::abs(chunk); ++k) iteration();
        capture_whole = 0;
        if (whole) {
          hipLaunchKernelGGL(k_solve_end_g, dim3(g), dim3(NT), 0, s, n, ws.st, ws.args_dev.p, (int)two_launch(), ws.x, ws.res_norm.p,
                             &ws.flags[0], &ws.st->x0_zero, ws.end_count.p);
          MI_HIP(hipGetLastError());
        }
      });
    } catch (...) {
      capture_whole = 0;
      throw;
    }
    ws.graphs[key] = ex;
    ++ctx->n_captures;
    return ex;
  }

  // Wait for the exit kernel of a whole-solve graph: it stores the solve number after everything else it wrote has been
  // released to system scope. A bounded spin (a replay that takes longer, or a fault, ends in a stream synchronisation).
  void wait_seq(unsigned long long seq) {
    volatile unsigned long long *f = &ws.flags[0].seq;
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned k = 1;; ++k) {
      if (*f == seq) { std::atomic_thread_fence(std::memory_order_acquire); return; }
      if ((k & 0xfff) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) break;
      __builtin_ia32_pause();
    }
    MI_HIP(hipStreamSynchronize(s));
    std::atomic_thread_fence(std::memory_order_acquire);
    if (*f != seq) raise(MI_ERR_HIP, "internal: the solve's exit kernel did not report (seq %llu, expected %llu)", (unsigned long long)*f, seq);
  }

  void fetch_flags(int slot) {
    MI_HIP(hipMemcpyAsync(&ws.flags[slot].it, two_launch() ? &ws.st->it_nxt : &ws.st->it, sizeof(long long),
                          hipMemcpyDeviceToHost, s));
    MI_HIP(hipMemcpyAsync(&ws.flags[slot].done, &ws.st->done, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    MI_HIP(hipEventRecord(ws.ev[slot], s));
  }

  // Common entry of every solver: b, x to the workspace; eps / maxit / res_cap to the state block; deflated
  // solvers: W, WtA, WtAW (LU on the host) and the deflated initial guess (defcg.jl:40-54 / 260-275).
  void begin(const double *b_in, const double *x_in, const double *W_in, int64_t &maxit, double &eps, int64_t &cap_dev) {
    prepare(maxit, eps, cap_dev);
    const size_t vb = sizeof(double) * (size_t)n;
    hipLaunchKernelGGL(k_solve_begin, dim3(g), dim3(NT), 0, s, n, b_in, x_in, ws.b, ws.x, ws.st, eps, (long long)maxit,
                       (long long)cap_dev);
    MI_HIP(hipGetLastError());
    if (nvec > 0) {
      MI_HIP(hipMemcpyAsync(ws.W.p, W_in, vb * nvec, hipMemcpyDeviceToDevice, s));
      if (folded()) {
        hipLaunchKernelGGL(k_gather_w_loc, dim3((Ad->maps.nloc + NT - 1) / NT, nvec), dim3(NT), 0, s, nvec, (long long)n, Ad->maps.nloc,
                           Ad->maps.gidx.p, ws.W.p, ws.fold_wloc.p);
        MI_HIP(hipGetLastError());
      }
      A->apply_multi(ws.W.p, n, nvec, ws.AW.p, n);                           // WtA[v,:] = A*W[:,v]
      hipLaunchKernelGGL(k_small_gram, dim3(nvec, nvec), dim3(NT), 0, s, n, ws.AW.p, ws.W.p, ws.gram.p, nvec);  // WtAW
      MI_HIP(hipGetLastError());
      factor(ws.gram.p, ws.LU, ws.piv, &gram_host, "WtAW");
      A->apply(ws.x, ws.Ap, nullptr);                                        // r .= b .- A*x
      hipLaunchKernelGGL(k_residual, dim3(g), dim3(NT), 0, s, n, ws.b, ws.Ap, ws.r, ws.part_rr, ws.part_bb);
      project(ws.W.p, ws.r, nullptr);                                        // mu = WtAW \ (W'r)
      hipLaunchKernelGGL(k_add_Wmu, dim3(g), dim3(NT), 0, s, n, ws.x, ws.W.p, ws.mu.p, nvec);  // x .+= W*mu
      MI_HIP(hipGetLastError());
    }
  }
  // host half of the entry: defaults, capacities, buffers
  void prepare(int64_t &maxit, double &eps, int64_t &cap_dev) {
    if (eps <= 0.0) eps = 1e-7;           // RecyclingKrylovSolvers.jl:21
    if (maxit == 0) maxit = n;            // cg.jl:25
    // reference: res_norm has n entries and `res_norm[it] = ...` throws BoundsError at it = n + 1 (cg.jl:23,47), which
    // only maxit > n can reach: the device loop stops there too (overflow flag -> MI_ERR_RES_CAPACITY), with x updated
    // exactly as often as the reference had updated it when it threw
    cap_dev = std::max<int64_t>(1, std::min<int64_t>(maxit, (int64_t)n));
    if ((size_t)cap_dev + 1 > ws.res_norm.n) { ws.drop_graphs(); ws.res_norm.alloc((size_t)cap_dev + 1); }
    if (nvec > 0) ws.ensure_deflation(nvec);
    if (nvec > 0 && folded()) {
      const size_t need_mu = (size_t)nvec * Md->ntiles + 1, need_wm = (size_t)Ad->maps.nloc + 1;
      const size_t need_wl = (size_t)nvec * Ad->maps.nloc + 1;
      if (ws.fold_mu.n < need_mu || ws.fold_wm.n < need_wm || ws.fold_wloc.n < need_wl) {
        ws.drop_graphs();  // buffers move
        ws.fold_mu.alloc(need_mu); ws.fold_wm.alloc(need_wm); ws.fold_wloc.alloc(need_wl);
      }
    }
    if (form == Loop::CSRFOLD) {
      const size_t need_pz = 4 * (size_t)n + 2, need_p = (size_t)CF_VEC_GRID + 1;
      if (ws.cf_pz.n < need_pz || ws.cf_rr.n < need_p) {
        ws.drop_graphs();  // buffers move
        ws.cf_pz.alloc(need_pz); ws.cf_rr.alloc(need_p); ws.cf_rz.alloc(need_p);
      }
    }
  }
  // LU (host, LAPACK getrf order) of the nvec x nvec device matrix `gram`; factors and pivots back to the device.
  void factor(const double *gram, DevBuf<double> &LU, DevBuf<int> &piv, std::vector<double> *keep, const char *name) {
    std::vector<double> lu((size_t)nvec * nvec);
    MI_HIP(hipMemcpyAsync(lu.data(), gram, sizeof(double) * lu.size(), hipMemcpyDeviceToHost, s));
    MI_HIP(hipStreamSynchronize(s));
    if (keep) *keep = lu;
    std::vector<int> pv;
    const int info = host_lu(nvec, lu, pv);
    if (info) raise(MI_ERR_SINGULAR, "%s is singular: U[%d,%d] == 0 (SingularException(%d))", name, info, info, info);
    LU.upload(lu.data(), lu.size(), s);
    piv.upload(pv.data(), pv.size(), s);
    MI_HIP(hipStreamSynchronize(s));
  }

  // b_in / x_io / W_in are device pointers here (host mode is staged by the caller).
  int solve(const double *b_in, double *x_io, const double *W_in, int64_t maxit, double eps, double *res_host,
            int64_t res_cap, int64_t *it_out) {
    int64_t cap_dev = 0;
    struct AbortFlag {   // peer exchange: a wait that expires during this solve sets the stop flag (no iterating on garbage up to maxit)
      mi_ctx_s *c; hipStream_t s;
      AbortFlag(mi_ctx_s *c_, hipStream_t s_, int *flag) : c(c_), s(s_) { if (c->use_peer()) c->peer->set_abort_flag(flag, s); }
      ~AbortFlag() { if (c->use_peer()) { c->peer->set_abort_flag(nullptr, s); (void)hipStreamSynchronize(s); } }
    } abort_flag(ctx, s, &ws.st->done);
    bool use_graph = ctx->chunk > 0 && A->graph_safe() && (!M || M->graph_safe()) && !ctx->no_graph;
    // Undeflated solves on one GPU: entry kernel, set-up, iterations and exit kernel are ONE graph replay whose per-call
    // arguments travel through a pinned block, and the host waits for the exit kernel's last store instead of the stream.
    const bool whole_on = !env_int("MI355_NO_WHOLE_GRAPH", 0);
    const bool whole = whole_on && use_graph && nvec == 0 && !eig.tag && !ctx->has_comm();
    if (whole) prepare(maxit, eps, cap_dev);
    else begin(b_in, x_io, W_in, maxit, eps, cap_dev);

    // ---- set-up tail + loop
    const int64_t ncap = std::min<int64_t>(res_cap, cap_dev);
    const bool spec_res = res_host && ncap > 0 && ncap <= RES_STAGE;
    auto enqueue_results = [&](int slot) {
      hipLaunchKernelGGL(k_solve_end, dim3(g), dim3(NT), 0, s, n, ws.st, (int)two_launch(), ws.x, x_io, ws.res_norm.p,
                         spec_res ? ws.res_stage : (double *)nullptr, (long long)ncap, &ws.flags[slot], &ws.st->x0_zero);
      MI_HIP(hipGetLastError());
    };
    if (use_graph) {
      const GraphKey pk{A, M, nvec, 0};
      int &predicted = ws.predicted[pk];
      // Exact prediction for short solves; long ones (hundreds of iterations, counts that drift from solve to
      // solve) round down to a multiple of 32 so that only a few graph sizes are ever instantiated.
      int64_t first = predicted > 0 ? predicted : ctx->chunk;
      if (first > 64) first -= first % 32;
      first = std::max<int64_t>(1, std::min<int64_t>(first, std::min<int64_t>(maxit, 1024)));
      if (ws.graphs.size() > 48) ws.drop_graphs();
      // folded loop: the entry for x0 == 0 when the previous solve with these operators had one (checked on the device)
      bool zero_variant = whole && form == Loop::FOLD && ws.zero_x0[pk] && !env_int("MI355_NO_ZERO_ENTRY", 0);
      hipGraphExec_t g0 = nullptr;
      try {
        g0 = graph(-(int)first, whole ? (zero_variant ? 2 : 1) : 0);
      } catch (const Error &) {
        // A collective that cannot be captured (communicator attached): run this context eagerly from now on.
        // Every rank takes the same path because capture fails or succeeds identically on all of them.
        if (!ctx->comm) throw;
        ctx->no_graph = true;
        use_graph = false;
      }
      if (use_graph) {
      if (whole) {
        const unsigned long long seq = ++ws.seq;
        *ws.args = SolveArgs{b_in, x_io, x_io, spec_res ? ws.res_stage : (double *)nullptr, eps, (long long)maxit, (long long)cap_dev,
                             (long long)ncap, seq};
        ++ctx->n_replays; MI_HIP(hipGraphLaunch(g0, s));
        wait_seq(seq);
        if (ws.flags[0].respec) {   // x0 was not zero after all: the general form, and no such guess next time
          zero_variant = false;
          ws.zero_x0[pk] = false;
          g0 = graph(-(int)first, 1);
          const unsigned long long seq2 = ++ws.seq;
          ws.args->seq = seq2;
          ++ctx->n_replays; MI_HIP(hipGraphLaunch(g0, s));
          wait_seq(seq2);
        }
        if (folded()) ws.zero_x0[pk] = ws.flags[0].x0z != 0;
        if (ws.stats_on) ws.stat(ws.flags[0].t_exit - ws.flags[0].t_entry);
        if (ws.fold_dbg.p && folded()) {   // stamps of the solve that has just finished (100 MHz ticks -> us since the first one)
          std::vector<long long> h(512);
          MI_HIP(hipStreamSynchronize(s));
          memcpy_sync(h.data(), ws.fold_dbg.p, 512 * sizeof(long long), hipMemcpyDeviceToHost);
          const long long t0 = h[0] ? h[0] : ws.flags[0].t_entry;
          std::fprintf(stderr, "[fold stamps] wg %d, entry kernel at %.2f us\n", env_int("MI355_FOLD_DEBUG_WG", 0), (ws.flags[0].t_entry - t0) * 0.01);
          for (int r = 0; r < 64 && h[r * 8]; ++r) {
            std::fprintf(stderr, "  launch %2d:", r);
            for (int k = 0; k < 7; ++k) std::fprintf(stderr, " %8.2f", h[r * 8 + k] ? (h[r * 8 + k] - t0) * 0.01 : -1.0);
            std::fprintf(stderr, "\n");
          }
          memset_sync(ws.fold_dbg.p, 0, 512 * sizeof(long long));
        }
      } else {
        ++ctx->n_replays; MI_HIP(hipGraphLaunch(g0, s));
        enqueue_results(0);
        MI_HIP(hipStreamSynchronize(s));
      }
      if (!ws.flags[0].done) {
        hipGraphExec_t ex = graph(ctx->chunk);
        const int64_t max_launch = (maxit + ctx->chunk - 1) / ctx->chunk + 2;
        int slot = 0;
        bool stop = false;
        fetch_flags(slot);
        for (int64_t l = 0; l < max_launch && !stop; ++l) {
          ++ctx->n_replays; MI_HIP(hipGraphLaunch(ex, s));
          const int prev = slot;
          slot ^= 1;
          fetch_flags(slot);
          MI_HIP(hipEventSynchronize(ws.ev[prev]));
          stop = ws.flags[prev].done != 0;
        }
        enqueue_results(0);
        MI_HIP(hipStreamSynchronize(s));
      }
      predicted = (int)std::max<long long>(1, ws.flags[0].it - (two_launch() ? 0 : 1));  // the two-launch forms check the stop rule one launch later
      }
    }
    if (!use_graph) {
      setup_tail();
      for (int64_t l = 0; l < maxit + 2; ++l) {
        fetch_flags(0);
        MI_HIP(hipEventSynchronize(ws.ev[0]));
        if (ws.flags[0].done) break;
        iteration();
      }
      enqueue_results(0);
      MI_HIP(hipStreamSynchronize(s));
    }
    const long long it = ws.flags[0].it;
    if (ctx->use_peer() && ctx->peer->take_error(s))
      raise(MI_ERR_COMM, "peer exchange: a wait for the other ranks expired (MI355_PEER_TIMEOUT_MS): %s; the iterates of this solve are not valid", ctx->peer->err_text.c_str());
    if (!ws.flags[0].done) raise(MI_ERR_HIP, "internal: Krylov loop ended without the stop flag (it=%lld)", it);
    const int64_t ncopy = std::min<int64_t>(it, ncap);
    if (res_host && ncopy > 0) {
      if (spec_res) std::memcpy(res_host, ws.res_stage, sizeof(double) * ncopy);
      else {
        MI_HIP(hipMemcpyAsync(res_host, ws.res_norm.p, sizeof(double) * ncopy, hipMemcpyDeviceToHost, s));
        MI_HIP(hipStreamSynchronize(s));
      }
    }
    if (it_out) *it_out = it;
    if (ws.flags[0].overflow || it > res_cap)
      return fail(MI_ERR_RES_CAPACITY, "res_norm capacity %lld < it = %lld", (long long)res_cap, it);
    return MI_OK;
  }
};

}  // namespace mi
